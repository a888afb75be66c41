"""The helper of the large-offset GPU tests (tests/large_offsets.py) on the host: its generators and references at small
sizes against naive numpy loops, the window arithmetic, the bounds that make the GPU comparisons exact, and the mutation
check -- at the very shapes tests/test_gpu_large_offsets.py uses, a reference whose flat index lost 2^30, 2^31 or 2^32
elements differs in every window row."""
import numpy as np
import pytest
import torch

from tests import large_offsets as L

# the shapes of tests/test_gpu_large_offsets.py
C = 1024
ROWS_FULL = 2 ** 22 + 64         # 2^32 + 65536 elements: crosses E30, E31 and E32
ROWS_HALF = 2 ** 21 + 64         # 2^31 + 65536 elements: crosses E30 and E31
M_TABLE = 4096


# ------------------------------------------------------------------------------------------------------------- windows
def test_windows_at_the_gpu_shapes():
    w = L.windows(ROWS_FULL, C)
    assert w == [(0, 64), (ROWS_FULL - 64, ROWS_FULL), (2 ** 20 - 64, 2 ** 20 + 65), (2 ** 21 - 64, 2 ** 21 + 65),
                 (2 ** 22 - 64, ROWS_FULL)]                       # the E32 window is cut off by the end of the array
    for E in L.BOUNDARIES:                                          # each boundary element lies in a window, with rows on both sides
        r = E // C
        assert any(lo <= r - 1 and r + 1 < hi for lo, hi in w)
    h = L.windows(ROWS_HALF, C)
    assert h == [(0, 64), (ROWS_HALF - 64, ROWS_HALF), (2 ** 20 - 64, 2 ** 20 + 65), (2 ** 21 - 64, ROWS_HALF)]     # E32: dropped
    rows = L.window_rows(ROWS_FULL, C)
    assert rows.dtype == np.int64 and (np.diff(rows) > 0).all() and rows[0] == 0 and rows[-1] == ROWS_FULL - 1
    assert rows.shape[0] == 64 + 129 + 129 + 128                    # the end window and the E32 window overlap


def test_windows_fall_off_the_end():
    assert L.windows(10, 4) == [(0, 10), (0, 10)]                   # shorter than a window: clipped, no boundary reached
    assert L.windows(0, 4) == [] and L.window_rows(0, 4).shape == (0,)
    # the boundary row is the last row / one past the last row / far past it
    rows = L.E30 // 1024
    assert L.windows(rows + 1, 1024)[2] == (rows - 64, rows + 1)
    assert L.windows(rows, 1024) == [(0, 64), (rows - 64, rows), (rows - 64, rows)]     # only the rows in front of it are left
    assert L.windows(rows - 64, 1024) == [(0, 64), (rows - 128, rows - 64)]
    # a narrow array: element E30 of a [.., 3] array is in row E30 // 3
    assert L.windows(2 ** 29, 3)[2] == (L.E30 // 3 - 64, L.E30 // 3 + 65)
    assert L.chunks(10, 4) == [(0, 4), (4, 8), (8, 10)] and L.chunks(0) == []
    assert all(k1 - k0 <= L.CHUNK_ROWS for k0, k1 in L.chunks(ROWS_FULL)) and len(L.chunks(ROWS_FULL)) == 17


# ------------------------------------------------------------------------------------------------------------ patterns
def test_float_patterns_against_loops():
    k = torch.tensor([0, 1, 60, 61, 62, 12345, 2 ** 22 + 63, 2 ** 31 - 1], dtype=torch.int64)
    Cs = 9
    v, g, t = L.value_pattern(k, Cs), L.grad_pattern(k, Cs), L.table_pattern(k[:6], Cs)
    for i, kk in enumerate(k.tolist()):
        for c in range(Cs):
            assert v[i, c] == (kk % 61) - 30 + (c % 7) and g[i, c] == (kk % 13) - 6 + (c % 3)
            if i < 6:
                assert t[i, c] == kk * Cs + c
    assert v.dtype == g.dtype == t.dtype == torch.float32
    big = torch.arange(0, 70000, dtype=torch.int64)
    assert float(L.value_pattern(big, 16).abs().max()) == L.VALUE_MAX and float(L.grad_pattern(big, 16).abs().max()) == L.GRAD_MAX
    w = L.weight_pattern(big)
    assert sorted(w.unique().tolist()) == [0.0, 1.0, 2.0] and float(w.max()) == L.WEIGHT_MAX
    # the table of the gather test holds its own flat index, exactly
    assert M_TABLE * C <= L.EXACT
    r = torch.tensor([0, 1, M_TABLE - 1], dtype=torch.int64)
    assert L.table_pattern(r, C)[2, C - 1] == M_TABLE * C - 1 and L.table_pattern(r, C).to(torch.int64)[1, 0] == C


def test_mix_is_the_same_for_tensors_arrays_and_ints():
    ks = [0, 1, 2, 749, 750, 2 ** 17, 2 ** 22 + 63, 2 ** 31 - 1]
    want = []
    for k in ks:                                                     # the definition, with Python's unbounded integers
        h = k * 0x9E3779B1
        assert h < 2 ** 63
        h = ((h ^ (h >> 15)) & 0x7FFFFFFF) * 0x2C1B3C6D
        assert h < 2 ** 63
        h ^= h >> 12
        want.append(h & 0x7FFFFFFF)
    assert [L.mix(k) for k in ks] == want
    assert L.mix(torch.tensor(ks, dtype=torch.int64)).tolist() == want
    assert L.mix(np.asarray(ks, np.int64)).tolist() == want


def test_row_pattern_against_a_loop_and_its_load():
    M, T = 64, 200000
    big = (1000, 5000, 17)                                          # row 17 is an odd row of [M / 4, M): empty but for these
    k = torch.arange(T, dtype=torch.int64)
    row = L.row_pattern(k, M, big)
    assert row.dtype == torch.int32
    for kk in list(range(0, 3000, 7)) + [T - 1]:
        want = 17 if 1000 <= kk < 6000 else L.row_pattern(kk, M)
        assert int(row[kk]) == want
        h = L.mix(kk)
        u, v = h % 1024, h >> 10
        plain = (v % 16) if u < 1000 else ((v % 2) * (M + 1) - 1 if u == 1023 else 16 + 2 * (v % 24))
        assert L.row_pattern(kk, M) == plain
    r = row.numpy().astype(np.int64)
    assert r.min() == -1 and r.max() == M                             # both out-of-range values occur
    counts = np.bincount(r[(r >= 0) & (r < M)], minlength=M)
    assert (counts[:16] > 256).all()                                  # long rows: chunks and a join
    assert (counts[16::2] > 0).all() and (counts[16::2] <= 256).all() # short rows
    odd = counts[17::2]
    assert counts[17] == 5000 and (np.delete(odd, 0) == 0).all()      # empty rows, and the one big row
    assert abs(int((r == -1).sum()) - int((r == M).sum())) < 60 and 120 < (r == -1).sum() + (r == M).sum() < 280
    # at the GPU test's shape the loads are what its docstring says (counted on a slice: the hash is uniform)
    rg = L.row_pattern(torch.arange(2 ** 20, dtype=torch.int64), M_TABLE).numpy().astype(np.int64)
    cg = np.bincount(rg[(rg >= 0) & (rg < M_TABLE)], minlength=M_TABLE)
    assert cg[:1024].min() * 4 > 256 and cg[1024::2].max() * 4 <= 256 and cg[1025::2].sum() == 0


def test_sparse_grad_rows():
    rows = L.sparse_grad_rows(ROWS_HALF, C)
    assert set(L.window_rows(ROWS_HALF, C).tolist()) <= set(rows.tolist()) and (np.diff(rows) > 0).all()
    assert 4099 in rows and 2 * 4099 in rows and rows.shape[0] < 1200
    assert all(4099 % (2 ** n) != 0 for n in range(1, 13))


# ---------------------------------------------------------------------------------------- the mutation: a wrapped index
@pytest.mark.parametrize("pattern", [L.value_pattern, L.grad_pattern, L.small_pattern, L.moment1_pattern, L.moment2_pattern],
                         ids=["value", "grad", "small", "moment1", "moment2"])
def test_a_wrapped_index_changes_every_window_row(pattern):
    """The 32-bit mutation of each GPU test's reference, at its own shape: the flat index less 2^30 (a byte offset that
    wraps at 4 GiB), 2^31 or 2^32.  Every window row behind the shift differs from the true row."""
    looked = L.assert_wrap_visible(pattern, ROWS_FULL, C)
    # the window rows behind E30, behind E31 and behind E32 (a boundary's own window: the boundary row and the 64 behind it)
    assert looked == (65 + 129 + 128 + 64) + (65 + 128 + 64) + (64 + 64)
    assert L.assert_wrap_visible(pattern, ROWS_HALF, C) == (65 + 128 + 64) + (64 + 64)      # the half shape: E30 and E31
    assert L.assert_wrap_visible(pattern, 1000, C) == 0                           # a small array crosses nothing
    # in closed form: a shift of whole rows moves k by shift / C, and 61, 13 and 5 divide no power of two
    for shift in L.BOUNDARIES:
        assert shift % C == 0 and (shift // C) % 61 != 0 and (shift // C) % 13 != 0 and (shift // C) % 5 != 0
    # rows that are no whole number of rows apart: the columns move too
    assert L.assert_wrap_visible(pattern, 2 ** 30 // 1000 + 70, 1000, shifts=(L.E30,)) > 0


def test_the_wrap_check_has_teeth():
    periodic = lambda k, Cc: ((k % 64)[:, None] + torch.arange(Cc)[None, :] % 7).to(torch.float32)      # noqa: E731
    with pytest.raises(AssertionError, match="look the same"):
        L.assert_wrap_visible(periodic, ROWS_FULL, C)
    # wrapped_rows against the definition, element by element
    pat, Cs, shift = L.value_pattern, 5, 13
    got = L.wrapped_rows(pat, 4, 8, Cs, shift)
    for k in range(4, 8):
        for c in range(Cs):
            e = k * Cs + c - shift
            assert got[k - 4, c] == ((e // Cs) % 61) - 30 + ((e % Cs) % 7)
    # the table of the gather test holds its flat index: any shift at all shows
    t = L.table_pattern(torch.arange(64, 80), C)
    assert not bool((t == L.wrapped_rows(L.table_pattern, 64, 80, C, 1)).any())


# ----------------------------------------------------------------------------------------------------- the 2^24 bounds
def test_the_bounds_that_make_the_gpu_comparisons_exact():
    """Every sum the GPU tests compare, at their shapes: terms times the largest magnitude of a term, below 2^24."""
    s = L.synthetic_samples(ROWS_FULL, ROWS_FULL, L.default_long_rays(ROWS_FULL, C), M=M_TABLE,
                            big_row=L.big_row_of(M_TABLE))
    counts = np.bincount(s.samples.row.numpy().astype(np.int64).clip(-1, M_TABLE) + 1, minlength=M_TABLE + 2)[1:M_TABLE + 1]
    assert counts[M_TABLE // 4 + 1] == L.LONG_RAY and counts.max() == L.LONG_RAY
    assert L.assert_exact(counts.max(), L.VALUE_MAX, "reduce_rows") == 4718592
    assert s.longest_ray == L.LONG_RAY
    assert L.assert_exact(s.longest_ray, L.VALUE_MAX, "ray_scan") == 4718592
    assert L.assert_exact(s.longest_ray, L.WEIGHT_MAX * L.VALUE_MAX, "accumulate") == 9437184
    assert L.assert_exact(C, L.GRAD_MAX * L.VALUE_MAX, "accumulate, grad_w") == 294912
    assert L.assert_exact(1, L.WEIGHT_MAX * L.GRAD_MAX, "accumulate, grad_values") == 16
    assert L.assert_exact(max(k1 - k0 for k0, k1 in s.ray_chunks), L.VALUE_MAX, "a chunk's cumsum") <= 4718592
    with pytest.raises(AssertionError, match="not below 2\\^24"):
        L.assert_exact(2 ** 19, L.VALUE_MAX, "too long")
    assert int(L.as_float32(torch.tensor([L.EXACT - 1])).item()) == L.EXACT - 1
    with pytest.raises(AssertionError):
        L.as_float32(torch.tensor([L.EXACT]))


# ------------------------------------------------------------------------------------------------------------- samples
def naive_lists(cuts, T):
    """offsets [T + 1] and ray [T] by a loop over the cuts."""
    offsets, ray = np.zeros(T + 1, np.int64), np.zeros(T, np.int64)
    ext = list(cuts) + [T]
    nxt = 0
    for q in range(T + 1):
        while ext[nxt] < q:
            nxt += 1
        offsets[q] = ext[nxt]
    for a, b in zip(ext[:-1], ext[1:]):
        ray[a:b] = a
    return offsets, ray


def test_synthetic_samples_small():
    T = 9000
    long_rays = [(3000, 2000), (6100, 200)]
    s = L.synthetic_samples(T, T, long_rays, M=32, big_row=(100, 700, 9), chunk=2048)
    S = s.samples
    assert len(S) == T and S.Q == T and S.offsets.dtype == torch.int64 and S.ray.dtype == S.row.dtype == torch.int32
    offsets, ray = naive_lists(s.cuts.tolist(), T)
    np.testing.assert_array_equal(S.offsets.numpy(), offsets)
    np.testing.assert_array_equal(S.ray.numpy(), ray)
    lengths = np.diff(offsets)
    assert lengths.sum() == T and offsets[0] == 0 and offsets[T] == T
    for n in (0, 1, 63, 64, 65, 257, 300, 2000, 200):
        assert (lengths == n).any(), n
    assert lengths[3000] == 2000 and lengths[6100] == 200 and s.longest_ray == 2000
    # every sample lies in the segment of the ray it names
    k = np.arange(T)
    assert (offsets[ray] <= k).all() and (k < offsets[ray + 1]).all()
    np.testing.assert_array_equal(S.row.numpy(), [9 if 100 <= kk < 800 else L.row_pattern(kk, 32) for kk in range(T)])
    # the chunks end on ray ends, cover everything, and hold whole rays only
    assert s.ray_chunks[0][0] == 0 and s.ray_chunks[-1][1] == T
    for (a, b), (c, _) in zip(s.ray_chunks, s.ray_chunks[1:] + [(T, T)]):
        assert b == c and 0 < b - a <= 2048 and (b == T or b in s.cuts)
        start, end = s.segment(a, b)
        assert int(start.min()) >= 0 and int(end.max()) <= b - a
        np.testing.assert_array_equal(start.numpy(), ray[a:b] - a)
        np.testing.assert_array_equal(end.numpy(), offsets[ray[a:b] + 1] - a)
    with pytest.raises(AssertionError, match="longer than a chunk"):
        L.synthetic_samples(T, T, long_rays, M=32, chunk=1024)


def test_synthetic_samples_straddle_the_boundary_rows():
    """At the GPU shapes: a ray of 2^17 samples, and a ray of 200 samples across each of the samples whose rows hold
    elements E31 and E32; the ray index runs with the sample index."""
    for rows, crossed, first in ((ROWS_FULL, (L.E31, L.E32), 750000), (ROWS_HALF, (L.E31,), 524250)):
        lr = L.default_long_rays(rows, C)
        assert lr[0] == (first, 2 ** 17) and first % L.PERIOD == 0 and len(lr) == 1 + len(crossed)
        cuts = L.ray_cuts(rows, lr)
        ext = np.concatenate([cuts, [rows]])
        assert cuts[0] == 0 and (np.diff(ext) > 0).all() and np.diff(ext).max() == 2 ** 17
        for E in crossed:
            s = E // C
            i = np.searchsorted(cuts, s, side="right") - 1
            assert cuts[i] == s - 100 and ext[i + 1] == min(s + 100, rows)      # samples on both sides of the boundary row
        i = np.searchsorted(cuts, first)
        assert cuts[i] == first and ext[i + 1] == first + 2 ** 17
        assert (np.diff(ext)[np.diff(ext) < 2 ** 17] <= 750).all()


# ---------------------------------------------------------------------------------------------------------- references
def test_references_against_loops():
    rng = np.random.default_rng(5)
    T, Cs, M = 700, 5, 11
    s = L.synthetic_samples(T, T, [(200, 130), (650, 200)], M=M, chunk=400)
    k = torch.arange(T, dtype=torch.int64)
    v = L.value_pattern(k, Cs)
    w = L.weight_pattern(k)
    row = s.samples.row
    ray = s.samples.ray
    vn, wn, rown, rayn = v.numpy().astype(np.int64), w.numpy().astype(np.int64), row.numpy(), ray.numpy()
    offsets = s.samples.offsets.numpy()

    table = torch.from_numpy(rng.standard_normal((M, Cs)).astype(np.float32))
    got = L.ref_gather(table, row)
    for kk in range(T):
        want = table[rown[kk]].numpy() if 0 <= rown[kk] < M else np.zeros(Cs, np.float32)
        np.testing.assert_array_equal(got[kk].numpy(), want)
    assert (rown == -1).any() or (rown == M).any()

    # sums, counts and maxima per row: in two chunks, as the GPU test feeds them
    acc = cnt = mx = None
    for a, b in ((0, 300), (300, T)):
        acc = L.ref_segment_sum(v[a:b], row[a:b], M, acc)
        cnt = L.ref_segment_count(row[a:b], M, cnt)
        mx = L.ref_segment_max(v[a:b], row[a:b], M, mx)
    for r in range(M):
        ks = np.nonzero(rown == r)[0]
        np.testing.assert_array_equal(acc[r].numpy(), vn[ks].sum(0))
        assert int(cnt[r]) == ks.shape[0]
        np.testing.assert_array_equal(mx[r].numpy(), vn[ks].max(0) if ks.shape[0] else np.full(Cs, -np.inf))
    assert acc.dtype == torch.int64 and (cnt == 0).any()

    # running sums within whole rays
    for a, b in s.ray_chunks:
        start, end = s.segment(a, b)
        for exclusive in (False, True):
            for reverse in (False, True):
                got = L.ref_segment_cumsum(v[a:b], start, end, exclusive, reverse).numpy()
                for q in np.unique(rayn[a:b]):
                    lo, hi = offsets[q], offsets[q + 1]
                    seg = vn[lo:hi][::-1] if reverse else vn[lo:hi]
                    run = np.cumsum(seg, axis=0)
                    if exclusive:
                        run = run - seg
                    np.testing.assert_array_equal(got[lo - a:hi - a], run[::-1] if reverse else run)

    # accumulate and its two gradients
    out = L.ref_accumulate(w, v, ray, T).numpy()
    g = L.grad_pattern(k, Cs)
    gn = g.numpy().astype(np.int64)
    gw, gv = L.ref_accumulate_grads(w, v, ray, g)
    want = np.zeros((T, Cs), np.int64)
    for kk in range(T):
        want[rayn[kk]] += wn[kk] * vn[kk]
        assert int(gw[kk]) == int((gn[rayn[kk]] * vn[kk]).sum())
        np.testing.assert_array_equal(gv[kk].numpy(), wn[kk] * gn[rayn[kk]])
    np.testing.assert_array_equal(out, want)
    # a sample whose ray is outside [0, Q) gets zeros
    bad = ray.clone()
    bad[3], bad[4] = -1, T
    gw, gv = L.ref_accumulate_grads(w, v, bad, g)
    assert int(gw[3]) == 0 and int(gw[4]) == 0 and not bool(gv[3:5].any()) and bool(gv[5:].any())
