"""RaySamples.split and merge_samples without a GPU: the C ABI's argument checks, the Python layer's, and the restatement
(tests/cut_restate.py) against a brute-force union, against its own identities and against float64."""
import ctypes

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from tests import cut_restate as X
from tests import samples_restate as R

NAMES = ("svoxt_samples_split_workspace_bytes", "svoxt_samples_split_count", "svoxt_samples_split_emit",
         "svoxt_samples_merge_workspace_bytes", "svoxt_samples_merge_count", "svoxt_samples_merge_emit")
F = np.float32


def test_symbols_and_abi_version():
    lib = ctypes.CDLL(_C.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _C.EXPORTS
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22
    for name in ("merge_samples", "take_samples"):
        assert callable(getattr(svox, name)) and name in svox.__all__
    assert callable(svox.RaySamples.split)
    for wb in (_C._lib.svoxt_samples_split_workspace_bytes, _C._lib.svoxt_samples_merge_workspace_bytes):
        assert wb(0) == 0 and wb(-1) == -1 and wb(1 << 31) == -1
        assert wb(1) > 0 and wb(1) % 256 == 0 and wb(100000) >= 2 * 4 * 100000


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _C._lib
    err = lib.svoxt_last_error
    buf = (ctypes.c_float * 400)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    p2 = ctypes.c_void_p(p.value + 256)
    p3 = ctypes.c_void_p(p.value + 512)
    p4 = ctypes.c_void_p(p.value + 768)
    odd4 = ctypes.c_void_p(p.value + 4)                # 4-byte aligned, not 8
    odd1 = ctypes.c_void_p(p4.value + 1)
    sc, se = lib.svoxt_samples_split_count, lib.svoxt_samples_split_emit
    mc, me = lib.svoxt_samples_merge_count, lib.svoxt_samples_merge_emit
    big = 1 << 20

    def split_count(length=p, pieces=None, max_length=0.5, max_pieces=4096, offsets=p2, Q=4, T=4, offsets_out=p3, total=p4, ws=p, nbytes=big):
        return sc(length, pieces, max_length, max_pieces, offsets, Q, T, offsets_out, total, ws, nbytes, None)

    def split_emit(T=4, ws=p, nbytes=big, ins=(p, p, p, p), T_out=6, outs=(p2, p2, p2, p2, p2)):
        return se(T, ws, nbytes, *ins, T_out, *outs, None)

    def merge_count(a=(p, p, p), Ta=4, b=(p2, p2, p2), Tb=4, Q=4, offsets_out=p3, total=p4, ws=p, nbytes=big):
        return mc(*a, Ta, *b, Tb, Q, offsets_out, total, ws, nbytes, None)

    def merge_emit(a=(p, p, p), Ta=4, b=(p2, p2, p2), Tb=4, Q=4, offsets_out=p3, T_out=6, outs=(p4, p4, p4, p4, p4, p4)):
        return me(*a, Ta, *b, Tb, Q, offsets_out, T_out, *outs, None)

    # extents
    for bad in (-1, 1 << 31):
        assert split_count(Q=bad) == 1 and b"svoxt_samples_split_count: Q must be in [0, 2^31)" in err()
        assert split_count(T=bad) == 1 and b"svoxt_samples_split_count: T must be in [0, 2^31)" in err()
        assert split_emit(T=bad) == 1 and b"svoxt_samples_split_emit: T must be in [0, 2^31)" in err()
        assert split_emit(T_out=bad) == 1 and b"svoxt_samples_split_emit: T_out must be in [0, 2^31)" in err()
        for kw in (dict(Q=bad), dict(Ta=bad), dict(Tb=bad)):
            assert merge_count(**kw) == 1 and b"svoxt_samples_merge_count: " in err() and b"must be in [0, 2^31)" in err()
            assert merge_emit(**kw) == 1 and b"svoxt_samples_merge_emit: " in err() and b"must be in [0, 2^31)" in err()
        assert merge_emit(T_out=bad) == 1 and b"svoxt_samples_merge_emit: T_out must be in [0, 2^31)" in err()
    assert split_emit(T=0, T_out=1) == 1 and b"0 for T = 0" in err()
    # how to cut
    assert split_count(max_length=0.0) == 1 and b"neither max_length nor pieces is given" in err()
    assert split_count(pieces=p2, max_length=0.5) == 1 and b"both max_length and pieces are given" in err()
    for ml in (-1.0, float("nan"), -float("inf")):
        assert split_count(max_length=ml) == 1 and b"svoxt_samples_split_count: max_length must be > 0" in err()
    for mp in (0, -1, (1 << 30) + 1):
        assert split_count(max_pieces=mp) == 1 and b"max_pieces must be in [1, 2^30]" in err()
    # NULL
    assert split_count(offsets_out=None) == 1 and b"svoxt_samples_split_count: offsets_out / total is NULL" in err()
    assert split_count(total=None) == 1 and b"svoxt_samples_split_count: offsets_out / total is NULL" in err()
    assert split_count(length=None) == 1 and b"svoxt_samples_split_count: length / offsets is NULL" in err()
    assert split_count(offsets=None) == 1 and b"svoxt_samples_split_count: length / offsets is NULL" in err()
    assert split_count(ws=None) == 1 and b"svoxt_samples_split_count: workspace is NULL" in err()
    for i in range(4):
        ins = tuple(None if j == i else p for j in range(4))
        assert split_emit(ins=ins) == 1 and b"svoxt_samples_split_emit: ray / row / depth / length is NULL" in err()
    for i in range(5):
        outs = tuple(None if j == i else p2 for j in range(5))
        assert split_emit(outs=outs) == 1 and b"svoxt_samples_split_emit: an output is NULL" in err()
    assert split_emit(ws=None) == 1 and b"svoxt_samples_split_emit: workspace is NULL" in err()
    assert merge_count(offsets_out=None) == 1 and b"svoxt_samples_merge_count: offsets_out / total is NULL" in err()
    assert merge_count(total=None) == 1 and b"svoxt_samples_merge_count: offsets_out / total is NULL" in err()
    for fn, name in ((merge_count, b"svoxt_samples_merge_count"), (merge_emit, b"svoxt_samples_merge_emit")):
        assert fn(a=(None, p, p)) == 1 and name + b": offsets_a / offsets_b is NULL" in err()
        assert fn(b=(None, p, p)) == 1 and name + b": offsets_a / offsets_b is NULL" in err()
        for side in ((p, None, p), (p, p, None)):
            assert fn(a=side) == 1 and name + b": depth / length of a list with samples is NULL" in err()
            assert fn(b=side) == 1 and name + b": depth / length of a list with samples is NULL" in err()
    assert merge_count(ws=None) == 1 and b"svoxt_samples_merge_count: workspace is NULL" in err()
    assert merge_emit(offsets_out=None) == 1 and b"svoxt_samples_merge_emit: offsets_out is NULL" in err()
    for i in range(6):
        outs = tuple(None if j == i else p4 for j in range(6))
        assert merge_emit(outs=outs) == 1 and b"svoxt_samples_merge_emit: an output is NULL" in err()
    # a short workspace
    need_s, need_m = lib.svoxt_samples_split_workspace_bytes(4), lib.svoxt_samples_merge_workspace_bytes(4)
    assert split_count(nbytes=need_s - 1) == 1 and b"svoxt_samples_split_count: workspace smaller" in err()
    assert split_emit(nbytes=need_s - 1) == 1 and b"svoxt_samples_split_emit: workspace smaller" in err()
    assert merge_count(nbytes=need_m - 1) == 1 and b"svoxt_samples_merge_count: workspace smaller" in err()
    # alignment
    assert split_count(offsets=odd4) == 1 and b"svoxt_samples_split_count: offsets is not 8-byte aligned" in err()
    assert split_count(offsets_out=odd4) == 1 and b"svoxt_samples_split_count: offsets_out / total is not 8-byte" in err()
    assert split_count(total=odd4) == 1 and b"svoxt_samples_split_count: offsets_out / total is not 8-byte" in err()
    assert split_count(length=odd1) == 1 and b"svoxt_samples_split_count: length / pieces is not 4-byte aligned" in err()
    assert split_count(pieces=odd1, max_length=0.0) == 1 and b"svoxt_samples_split_count: length / pieces is not 4-byte aligned" in err()
    assert split_count(ws=odd4) == 1 and b"svoxt_samples_split_count: workspace is not 8-byte aligned" in err()
    for i in range(4):
        ins = tuple(odd1 if j == i else p for j in range(4))
        assert split_emit(ins=ins) == 1 and b"svoxt_samples_split_emit: a misaligned argument" in err()
    for i in range(5):
        outs = tuple((odd4 if i == 4 else odd1) if j == i else p2 for j in range(5))
        assert split_emit(outs=outs) == 1 and b"svoxt_samples_split_emit: a misaligned argument" in err()
    assert split_emit(ws=odd4) == 1 and b"svoxt_samples_split_emit: workspace is not 8-byte aligned" in err()
    for fn, name in ((merge_count, b"svoxt_samples_merge_count"), (merge_emit, b"svoxt_samples_merge_emit")):
        for side in ((odd4, p, p), (p, odd1, p), (p, p, odd1)):
            assert fn(a=side) == 1 and name + b": a misaligned argument" in err()
            assert fn(b=side) == 1 and name + b": a misaligned argument" in err()
    assert merge_count(offsets_out=odd4) == 1 and b"svoxt_samples_merge_count: offsets_out / total is not 8-byte" in err()
    assert merge_count(total=odd4) == 1 and b"svoxt_samples_merge_count: offsets_out / total is not 8-byte" in err()
    assert merge_count(ws=odd4) == 1 and b"svoxt_samples_merge_count: workspace is not 8-byte aligned" in err()
    assert merge_emit(offsets_out=odd4) == 1 and b"svoxt_samples_merge_emit: a misaligned argument" in err()
    for i in range(6):
        outs = tuple((odd1 if i < 4 else odd4) if j == i else p4 for j in range(6))
        assert merge_emit(outs=outs) == 1 and b"svoxt_samples_merge_emit: a misaligned argument" in err()
    # overlap
    assert split_count(offsets_out=p2) == 1 and b"svoxt_samples_split_count: offsets_out overlaps offsets" in err()
    assert merge_count(offsets_out=p) == 1 and b"svoxt_samples_merge_count: offsets_out overlaps offsets_a / offsets_b" in err()
    assert merge_count(offsets_out=p2) == 1 and b"svoxt_samples_merge_count: offsets_out overlaps offsets_a / offsets_b" in err()
    # nothing to emit is a valid no-op
    assert split_emit(T_out=0, ws=None, nbytes=0, ins=(None,) * 4, outs=(None,) * 5) == 0
    assert split_emit(T=0, T_out=0, ws=None, nbytes=0, ins=(None,) * 4, outs=(None,) * 5) == 0
    assert merge_emit(T_out=0, a=(None,) * 3, b=(None,) * 3, offsets_out=None, outs=(None,) * 6) == 0
    assert merge_emit(Q=0, a=(None,) * 3, b=(None,) * 3, offsets_out=None, outs=(None,) * 6) == 0


def cpu_samples(T=6, Q=3):
    off = torch.tensor([0, 2] + [2] * (Q - 2) + [T], dtype=torch.int64)
    return svox.RaySamples(off, torch.zeros(T, dtype=torch.int32), torch.zeros(T, dtype=torch.int32), torch.zeros(T), torch.ones(T))


def test_python_layer_checks_arguments_before_the_device():
    s = cpu_samples()
    ones = torch.ones(6, dtype=torch.int32)
    for kw in (dict(), dict(max_length=0.5, pieces=ones)):
        with pytest.raises(RuntimeError, match="exactly one of max_length and pieces"):
            s.split(**kw)
    for ml in (0, 0.0, -1.0, float("nan"), "long", torch.tensor(0.5), True):
        with pytest.raises(RuntimeError, match="max_length must be a float > 0"):
            s.split(ml)
    for pc in (torch.ones(5, dtype=torch.int32), torch.ones(6, dtype=torch.int64), torch.ones(6), torch.ones(6, 1, dtype=torch.int32), [1] * 6):
        with pytest.raises(RuntimeError, match=r"pieces must be int32 \[T\]"):
            s.split(pieces=pc)
    for mp in (0, -1, (1 << 30) + 1, 2.0, True, None):
        with pytest.raises(RuntimeError, match="max_pieces must be an int in"):
            s.split(0.5, max_pieces=mp)
    with pytest.raises(RuntimeError, match="GPU"):
        s.split(0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        s.split(pieces=ones)
    with pytest.raises(RuntimeError, match="they must be lists of the same rays"):
        svox.merge_samples(s, cpu_samples(Q=4))
    for a, b in ((s, None), ((s.offsets,), s)):
        with pytest.raises(RuntimeError, match="a and b must be RaySamples"):
            svox.merge_samples(a, b)
    with pytest.raises(RuntimeError, match="GPU"):
        svox.merge_samples(s, cpu_samples())
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C._extras.samples_split(s.offsets, s.ray, s.row, s.depth, s.length, 0.5)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C._extras.samples_merge(s.offsets, s.depth, s.length, s.offsets, s.depth, s.length)


def test_take_samples_never_wraps():
    v = torch.arange(12, dtype=torch.float32).reshape(4, 3).requires_grad_(True)
    idx = torch.tensor([3, -1, 0, -1, 3], dtype=torch.int64)
    out = svox.take_samples(v, idx)
    assert out.shape == (5, 3)
    assert torch.equal(out.detach(), torch.stack([v[3], torch.zeros(3), v[0], torch.zeros(3), v[3]]).detach())
    out.sum().backward()
    assert torch.equal(v.grad, torch.tensor([[1.0] * 3, [0.0] * 3, [0.0] * 3, [2.0] * 3]))
    flat = svox.take_samples(torch.tensor([5.0, 7.0]), idx.clamp(max=1), fill=-2.0)
    assert flat.tolist() == [7.0, -2.0, 5.0, -2.0, 7.0]
    none = svox.take_samples(torch.zeros(0, 2), torch.tensor([-1, -1]), fill=1.5)
    assert none.shape == (2, 2) and bool((none == 1.5).all())
    for bad in (torch.tensor([0, 1], dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int64), [0, 1]):
        with pytest.raises(RuntimeError, match=r"index must be int64"):
            svox.take_samples(torch.ones(3), bad)


# ------------------------------------------------------------------------------------------------------- the restatement
def dyadic_lists(rng, Q, most=7, grid=64, span=4):
    """Lists whose samples do not overlap and whose breakpoints are multiples of 1 / grid in [0, span): exact in float32.
    Per ray sorted distinct grid points, and each interval between two neighbours is a sample or not: neighbours abut."""
    depth, length, counts = [], [], []
    for _ in range(Q):
        n = int(rng.integers(0, most + 1))
        pts = np.sort(rng.choice(grid * span, size=int(rng.integers(n + 1, 2 * n + 2)), replace=False)) / grid
        take = np.sort(rng.choice(len(pts) - 1, size=min(n, len(pts) - 1), replace=False)) if n else np.zeros(0, dtype=np.int64)
        depth.extend(pts[take])
        length.extend(pts[take + 1] - pts[take])
        counts.append(len(take))
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    T = int(offsets[-1])
    ray = np.repeat(np.arange(Q), counts).astype(np.int32)
    return R.Lists(offsets, rng.integers(0, 99, T).astype(np.int32), ray, np.array(depth, dtype=F), np.array(length, dtype=F))


def empty_lists(Q):
    return R.Lists(np.zeros(Q + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=F), np.zeros(0, dtype=F))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def assert_lists_bits(got, want):
    for g, w, name in zip(got, want, R.Lists._fields):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        np.testing.assert_array_equal(bits(g), bits(w), err_msg=name)


_PAIR = {}


def pair():
    """3 000 random rays of 0 .. 7 samples a list on dyadic breakpoints, and their merge: made once."""
    if not _PAIR:
        rng = np.random.default_rng(2027)
        a, b = dyadic_lists(rng, 3000), dyadic_lists(rng, 3000)
        _PAIR["v"] = (a, b) + X.merge(a, b)
    return _PAIR["v"]


def test_restated_merge_is_the_brute_force_union():
    a, b, m, ia, ib = pair()
    want = X.union(a, b)
    both = 0
    for q in range(len(a.offsets) - 1):
        lo, hi = int(m.offsets[q]), int(m.offsets[q + 1])
        got = [(float(m.depth[k]), int(ia[k]), int(ib[k])) for k in range(lo, hi)]
        assert got == want[q], q
        both += sum(1 for g in got if g[1] >= 0 and g[2] >= 0)
    assert both > 1000 and (m.row == -1).all() and np.array_equal(m.ray, np.repeat(np.arange(3000), np.diff(m.offsets)))


def assert_tiles(m, index, src):
    """The pieces with index == k tile [s_k, e_k): exact on dyadic breakpoints."""
    order = np.argsort(index, kind="stable")
    order = order[index[order] >= 0]
    k = index[order]
    first = np.concatenate([[True], k[1:] != k[:-1]])
    last = np.concatenate([k[1:] != k[:-1], [True]])
    end = (m.depth[order] + m.length[order]).astype(F)
    assert np.array_equal(np.unique(k), np.arange(len(src.depth)))                   # every sample is covered
    assert np.array_equal(m.depth[order][first], src.depth)
    assert np.array_equal(end[last], (src.depth + src.length).astype(F))
    assert np.array_equal(m.depth[order][1:][~first[1:]], end[:-1][~last[:-1]])      # each starts where the previous one ends


def test_restated_merge_tiles_every_sample_and_keeps_the_cap():
    a, b, m, ia, ib = pair()
    assert_tiles(m, ia, a)
    assert_tiles(m, ib, b)
    cap = 2 * (np.diff(a.offsets) + np.diff(b.offsets))
    assert (np.diff(m.offsets) <= cap).all() and ((ia >= 0) | (ib >= 0)).all()
    assert (np.diff(m.depth)[np.diff(m.ray) == 0] > 0).all()                         # monotone: these lists do not overlap themselves


def test_restated_merge_identities():
    a, b, _, _, _ = pair()
    none = empty_lists(3000)
    for first in (True, False):
        m, ia, ib = X.merge(a, none) if first else X.merge(none, a)
        assert_lists_bits(m._replace(row=a.row), a)
        mine, other = (ia, ib) if first else (ib, ia)
        assert np.array_equal(mine, np.arange(len(a.depth))) and (other == -1).all()
    m, ia, ib = X.merge(a, a)
    assert_lists_bits(m._replace(row=a.row), a)
    assert np.array_equal(ia, np.arange(len(a.depth))) and np.array_equal(ia, ib)
    m, ia, ib = X.merge(none, none)
    assert len(m.depth) == 0 and (m.offsets == 0).all()
    # lists that overlap themselves by a unit in the last place, as the march's do: still the list itself
    rng = np.random.default_rng(5)
    length = rng.uniform(0.01, 0.05, 400).astype(F)
    depth = (10 + np.cumsum(length) - length).astype(F)
    c = R.Lists(np.array([0, 150, 150, 400]), np.zeros(400, dtype=np.int32), np.repeat([0, 2], [150, 250]).astype(np.int32), depth, length)
    assert ((depth[:-1] + length[:-1]).astype(F) > depth[1:]).sum() > 20
    for other in (c, empty_lists(3)):
        m, ia, ib = X.merge(c, other)
        assert_lists_bits(m._replace(row=c.row), c)
        assert np.array_equal(ia, np.arange(400))


def test_restated_merge_degenerate_samples_stand_alone():
    """A sample with e > s false is emitted whole, alone, A's before B's, and cuts nothing."""
    nan = F(np.nan)
    a = R.Lists(np.array([0, 4]), np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32),
                np.array([0.0, 0.5, 0.5, nan], dtype=F), np.array([1.0, 0.0, -0.25, 1.0], dtype=F))
    b = R.Lists(np.array([0, 2]), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32),
                np.array([0.25, 0.75], dtype=F), np.array([nan, 1.0], dtype=F))
    m, ia, ib = X.merge(a, b)
    # B's degenerate sample is current from the start: it goes first; then A [0, 1) against B [0.75, 1.75)
    assert ia.tolist() == [-1, 0, 0, 1, 2, 3, -1] and ib.tolist() == [0, -1, 1, -1, -1, -1, 1]
    np.testing.assert_array_equal(bits(m.depth), bits(np.array([0.25, 0.0, 0.75, 0.5, 0.5, nan, 1.0], dtype=F)))
    np.testing.assert_array_equal(bits(m.length), bits(np.array([nan, 0.75, 0.25, 0.0, -0.25, 1.0, 0.75], dtype=F)))


def test_restated_split():
    rng = np.random.default_rng(11)
    T = 500
    length = rng.uniform(0.001, 3.0, T).astype(F)
    length[::50] = 0.0
    length[7::50] = -1.0
    length[9::50] = np.nan
    depth = rng.uniform(0, 100, T).astype(F)
    offsets = np.array([0, 0, 100, 100, 499, 500, 500], dtype=np.int64)
    ray = np.repeat(np.arange(6), np.diff(offsets)).astype(np.int32)
    row = rng.integers(0, 99, T).astype(np.int32)
    src = R.Lists(offsets, row, ray, depth, length)
    good = length > 0
    for kw in (dict(max_length=0.37), dict(max_length=1e-5), dict(pieces=rng.integers(-3, 40, T).astype(np.int32)),
               dict(pieces=np.full(T, 100000, dtype=np.int32), max_pieces=7)):
        o, r, w, z, d, index = X.split(offsets, ray, row, depth, length, **kw)
        m = np.bincount(index, minlength=T)
        assert np.array_equal(m, X.split_counts(length, **kw)) and (m >= 1).all() and (m[~good] == 1).all()
        assert m.max() <= kw.get("max_pieces", 4096) and np.array_equal(index, np.sort(index))
        assert np.array_equal(r, ray[index]) and np.array_equal(w, row[index])
        assert np.array_equal(o, np.concatenate([[0], np.cumsum(m)])[offsets])
        total = np.zeros(T)
        np.add.at(total, index, d.astype(np.float64))
        assert (np.abs(total - length)[good] <= ((m + 1) * 2.0 ** -24 * length)[good]).all()
        if "max_length" in kw:
            hit = m == kw.get("max_pieces", 4096)
            # no piece longer (a quotient that rounds down to an integer may leave it a unit in the last place longer), unless max_pieces stopped it
            assert (d[~hit[index] & good[index]] <= kw["max_length"] * (1 + 2.0 ** -22)).all()
        one = m[index] == 1
        np.testing.assert_array_equal(bits(d[one]), bits(length[index][one]))
        np.testing.assert_array_equal(bits(z[one]), bits(depth[index][one]))
        firsts = np.concatenate([[0], np.cumsum(m)[:-1]])
        assert np.array_equal(z[firsts][good], depth[good])                          # piece 0 starts at the sample
    assert X.split_counts(length, max_length=1e-5).max() == 4096 and X.split_counts(length, max_length=0.37).max() == 9
    assert X.split_counts(length, pieces=np.full(T, 100000, dtype=np.int32), max_pieces=7).max() == 7
    for kw in (dict(max_length=np.inf), dict(pieces=np.ones(T, dtype=np.int32)), dict(pieces=np.zeros(T, dtype=np.int32)),
               dict(max_length=3.5)):
        o, r, w, z, d, index = X.split(offsets, ray, row, depth, length, **kw)
        assert_lists_bits(R.Lists(o, w, r, z, d), src)
        assert np.array_equal(index, np.arange(T))


def take(values, index):
    return np.where(index >= 0, values[np.maximum(index, 0)], F(0)).astype(F)


def mixture(a, sa, b, sb, m, ia, ib):
    """(alpha32 over the merged lists with sigma_a + sigma_b, alpha64 = 1 - (1 - alpha_a)(1 - alpha_b), the bound)."""
    sm = (take(sa, ia) + take(sb, ib)).astype(F)
    alpha32 = R.weights(m.length, sm, m.offsets, torch.float32)[1].numpy().astype(np.float64)
    ta = 1.0 - R.weights(a.length, sa.astype(np.float64), a.offsets, torch.float64)[1].numpy()
    tb = 1.0 - R.weights(b.length, sb.astype(np.float64), b.offsets, torch.float64)[1].numpy()
    return alpha32, 1.0 - ta * tb, X.alpha_bound(m, sm, a, sa, b, sb)


def test_mixture_alpha_float32_against_the_float64_product():
    """The restated sample_weights over the merged lists with sigma_a + sigma_b against 1 - (1 - alpha_a)(1 - alpha_b) in
    float64: within half of cut_restate's bound, on dyadic lists and on lists far from the origin whose ends round."""
    a, b, m, ia, ib = pair()
    rng = np.random.default_rng(3)
    worst = 0.0
    cases = [(a, b, m, ia, ib)]
    length = rng.uniform(0.01, 0.05, 2000).astype(F)
    depth = (np.cumsum(length) - length).astype(F)
    counts = np.array([0, 1, 2, 63, 64, 65, 0, 0, 300, 505])
    off = np.concatenate([[0], np.cumsum(counts), np.cumsum(counts)[-1] + np.cumsum(counts)]).astype(np.int64)
    ray = np.repeat(np.arange(20), np.diff(off)).astype(np.int32)
    c = R.Lists(off, np.zeros(2000, dtype=np.int32), ray, depth, length)
    d = c._replace(depth=(depth + F(0.013)).astype(F), length=(length * F(0.9)).astype(F))
    cases.append((c, d) + X.merge(c, d))
    for (p, q, mm, ja, jb), scale in zip(cases, (8.0, 3.0)):
        sp = rng.uniform(0.05, scale, len(p.depth)).astype(F)
        sq = rng.uniform(0.05, scale, len(q.depth)).astype(F)
        got, want, bound = mixture(p, sp, q, sq, mm, ja, jb)
        ratio = np.abs(got - want) / bound
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 0.5).all(), float(ratio.max())
        assert 0.05 < want.mean() < 0.99 and (want > 0.5).sum() > 5
    print(f"mixture alpha: worst |alpha32 - alpha64| / bound = {worst:.3f}")


def test_split_alpha_against_the_lists_it_came_from():
    rng = np.random.default_rng(4)
    a = pair()[0]
    sigma = rng.uniform(0.05, 8.0, len(a.depth)).astype(F)
    o, r, w, z, d, index = X.split(a.offsets, a.ray, a.row, a.depth, a.length, max_length=0.11)
    assert len(index) > 1.5 * len(a.depth)
    coarse = R.weights(a.length, sigma, a.offsets, torch.float32)[1].numpy().astype(np.float64)
    fine = R.weights(d, sigma[index], o, torch.float32)[1].numpy().astype(np.float64)
    ratio = np.abs(fine - coarse) / X.split_alpha_bound(a, sigma, o, sigma[index])
    assert (ratio <= 1.0).all() and (fine != coarse).any()
    print(f"split alpha: worst |alpha32(split) - alpha32| / bound = {float(ratio.max()):.3f}")
