"""The flat-indexed operators on arrays of more than 2^31 and 2^32 elements ("Large offsets").

Shapes: rows of C = K = 1024 floats keep the counts small.  FULL = 2^22 + 64 rows is 2^32 + 65536 elements (16 GiB + 256
KiB) and crosses the elements 2^30 (a byte offset of 4 GiB), 2^31 and 2^32; where three or more arrays of that size
would be live at once, HALF = 2^21 + 64 rows (2^31 + 65536 elements, 8 GiB) crosses the first two.  A launch of a lane
per element of a FULL array has more than 2^32 lanes.

Inputs and references are tests/large_offsets.py's: closed-form integer patterns of the absolute index, generated and
generated again a chunk of at most 2^18 rows at a time, and exact references -- every comparison is an equality (see
that module for why that is sound, and tests/test_large_offsets_host.py for the bounds and for the 32-bit mutation of
each reference).  All of every output is compared, on the device; only window rows and small tables come to the host.

Every test states the bytes it needs, skips when the device cannot give them (plus 4 GiB), stays below 40 GiB, frees
what it allocated and prints its peak and its wall time (pytest -s shows them).  Run the tests one process each: the
first fault then ends the job."""
import functools
import gc
import time

import numpy as np
import pytest
import torch

import svox_t_amd as svox
from svox_t_amd import synth
from tests import large_offsets as L
from tests import optim_restate as OR

pytestmark = pytest.mark.gpu

C = 1024
FULL = 2 ** 22 + 64
HALF = 2 ** 21 + 64
M_TABLE = 4096
GIB = 2 ** 30
FULL_BYTES = FULL * C * 4
HALF_BYTES = HALF * C * 4
LIMIT = 40 * GIB
BIG_ROW = L.big_row_of(M_TABLE)[2]    # an odd row of [M / 4, M): empty but for its 2^17 samples


def large(need_bytes):
    """A test that needs `need_bytes` of device memory: skip without them (+ 4 GiB), report peak and time, give all back."""
    def deco(fn):
        @functools.wraps(fn)
        def run(gpu, *args, **kwargs):
            need = int(need_bytes)
            assert need <= LIMIT, f"{fn.__name__} plans {need / GIB:.1f} GiB: no test may need more than 40 GiB"
            gc.collect()
            torch.cuda.empty_cache()
            free, _ = torch.cuda.mem_get_info()
            if free < need + 4 * GIB:
                pytest.skip(f"{fn.__name__} needs {need / GIB:.1f} GiB + 4 GiB, the device has {free / GIB:.1f} GiB free")
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            try:
                fn(gpu, *args, **kwargs)
            finally:
                torch.cuda.synchronize()
                dt, peak = time.perf_counter() - t0, torch.cuda.max_memory_allocated()
                gc.collect()
                torch.cuda.empty_cache()
                what = fn.__name__ + ("[" + "-".join(str(a) for a in list(args) + list(kwargs.values())) + "]" if args or kwargs else "")
                print(f"\n[large offsets] {what}: peak {peak / GIB:.2f} GiB (planned {need / GIB:.2f}), {dt:.1f} s")
            assert peak <= LIMIT, f"peak device memory {peak / GIB:.2f} GiB is above 40 GiB"
        return run
    return deco


def rows_of(k0, k1, gpu):
    return torch.arange(k0, k1, dtype=torch.int64, device=gpu)


def filled(rows, pattern, gpu):
    """float32 [rows, C] on the device holding `pattern`, written a chunk at a time."""
    out = torch.empty((rows, C), dtype=torch.float32, device=gpu)
    for k0, k1 in L.chunks(rows):
        out[k0:k1] = pattern(rows_of(k0, k1, gpu), C)
    return out


def lists(rows, gpu, big_row=False):
    """The hand-made lists of `rows` samples over as many rays (tests/large_offsets.py: Synthetic)."""
    big = L.big_row_of(M_TABLE) if big_row else None
    return L.synthetic_samples(rows, rows, L.default_long_rays(rows, C), M=M_TABLE, big_row=big, device=gpu)


def assert_chunks_equal(got, chunk_refs, what, bits=False):
    """got [rows, C] against (k0, k1, expected) chunk by chunk, on the device; the first differing row goes to the host."""
    bad = None
    for k0, k1, want in chunk_refs:
        g = got[k0:k1]
        assert want.shape == g.shape and want.dtype == g.dtype, (what, want.shape, g.shape, want.dtype)
        same = torch.equal(g.view(torch.int32), want.view(torch.int32)) if bits else torch.equal(g, want)
        if not same and bad is None:
            r = int(torch.nonzero((g != want).any(dim=1))[0, 0]) if not bits else \
                int(torch.nonzero((g.view(torch.int32) != want.view(torch.int32)).any(dim=1))[0, 0])
            bad = (k0 + r, g[r].cpu().numpy(), want[r].cpu().numpy())
        del want
    if bad is not None:
        row, g, w = bad
        cols = np.nonzero(g.view(np.int32) != w.view(np.int32))[0]
        raise AssertionError(f"{what}: row {row} (element {row * got.shape[1]}) differs in {cols.shape[0]} columns, first "
                             f"column {cols[0]}: got {g[cols[0]]}, expected {w[cols[0]]}")


# ---------------------------------------------------------------------------------------------------------- gather_rows
@pytest.mark.parametrize("kernel", ["float4", "scalar"])
@large(FULL_BYTES + 3 * GIB)
def test_gather_rows(gpu, kernel):
    """Both kernels at 2^32 + 65536 output elements: all columns of a 16-byte aligned table (a lane per four columns), and
    `dim` a permutation of all 1024 columns (a lane per element: more than 2^32 lanes).  table[r, c] = 1024 r + c."""
    s = lists(FULL, gpu)
    table = L.table_pattern(rows_of(0, M_TABLE, gpu), C)
    assert table.data_ptr() % 16 == 0
    perm = (torch.arange(C, dtype=torch.int64) * 389 + 17) % C                   # 389 is odd: a permutation
    assert perm.unique().numel() == C
    dim = None if kernel == "float4" else perm
    out = svox.gather_rows(s.samples, table, dim=dim)
    assert out.shape == (FULL, C) and out.dtype == torch.float32 and out.data_ptr() % 16 == 0
    perm_d = perm.to(gpu)

    def refs():
        for k0, k1 in L.chunks(FULL):
            ref = L.ref_gather(table, s.samples.row[k0:k1])
            yield k0, k1, (ref if dim is None else ref[:, perm_d])
    assert_chunks_equal(out, refs(), f"gather_rows, {kernel} kernel", bits=True)
    # the window rows on the host, against plain numpy indexing
    w = L.window_rows(FULL, C)
    row = s.samples.row[torch.from_numpy(w).to(gpu)].cpu().numpy().astype(np.int64)
    inside = (row >= 0) & (row < M_TABLE)
    want = np.where(inside[:, None], row.clip(0, M_TABLE - 1)[:, None] * C + (np.arange(C) if dim is None else perm.numpy())[None, :], 0)
    np.testing.assert_array_equal(out[torch.from_numpy(w).to(gpu)].cpu().numpy(), want.astype(np.float32))
    assert inside.any() and (~inside).any()                              # rows outside the table occur among them


# --------------------------------------------------------------------------------- reduce_rows and gather_rows' backward
@large(2 * FULL_BYTES + 3 * GIB)
def test_reduce_rows_and_gather_backward(gpu):
    """sum, mean and max over values [2^22 + 64, 1024], and the gradient of gather_rows (the sum of a [T, 1024] upstream
    gradient): all of [M, 1024] against the exact reference, with long rows, short rows, empty rows (`empty`) and one row
    of 2^17 samples."""
    s = lists(FULL, gpu, big_row=True)
    S, row, M = s.samples, s.samples.row, M_TABLE
    values = filled(FULL, L.value_pattern, gpu)
    total = count = best = None
    for k0, k1 in L.chunks(FULL, L.CHUNK_ROWS // 2):
        total = L.ref_segment_sum(values[k0:k1], row[k0:k1], M, total)
        count = L.ref_segment_count(row[k0:k1], M, count)
        best = L.ref_segment_max(values[k0:k1], row[k0:k1], M, best)
    n = count.cpu().numpy()
    assert n[BIG_ROW] == L.LONG_RAY == n.max() and (n[:M // 4] > 256).all() and (n[M // 4::2] <= 256).all() and (n[M // 4::2] > 0).all()
    assert (np.delete(n[M // 4 + 1::2], 0) == 0).all()                            # the empty rows
    L.assert_exact(n.max(), L.VALUE_MAX, "reduce_rows")
    plan = S.row_plan(M)
    assert plan.longest == L.LONG_RAY and plan.n_outside == FULL - int(n.sum()) and plan.n_outside > 1000
    has = (count > 0)[:, None]
    want_sum = L.as_float32(total)

    got = svox.reduce_rows(S, values, M, "sum", empty=-7.0)
    assert torch.equal(got, torch.where(has, want_sum, torch.full_like(want_sum, -7.0))), "reduce_rows sum"
    got = svox.reduce_rows(S, values, M, "max", empty=5.5)
    assert torch.equal(got, torch.where(has, best, torch.full_like(best, 5.5))), "reduce_rows max"
    # the mean: one correctly rounded float32 division of two exact values, formed on the host
    got = svox.reduce_rows(S, values, M, "mean", empty=-7.0).cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        want = (want_sum.cpu().numpy() / n.astype(np.float32)[:, None]).astype(np.float32)
    np.testing.assert_array_equal(got, np.where(n[:, None] > 0, want, np.float32(-7.0)))
    del got
    # gather_rows' gradient: the same sums through autograd, rows without a sample get 0
    table = torch.zeros((M, C), dtype=torch.float32, device=gpu, requires_grad=True)
    out = svox.gather_rows(S, table)
    out.backward(values)
    del out
    assert torch.equal(table.grad, want_sum), "the gradient of gather_rows"


# ----------------------------------------------------------------------------------------------------------- accumulate
def weights_of(rows, gpu):
    return L.weight_pattern(rows_of(0, rows, gpu))


@large(2 * FULL_BYTES + 6 * GIB)
def test_accumulate_forward(gpu):
    """out [Q, 1024] with Q = 2^22 + 64: a lane per output element, more than 2^32 lanes; w in {0, 1, 2}."""
    s = lists(FULL, gpu)
    S = s.samples
    values, w = filled(FULL, L.value_pattern, gpu), weights_of(FULL, gpu)
    L.assert_exact(s.longest_ray, L.WEIGHT_MAX * L.VALUE_MAX, "accumulate")
    out = svox.accumulate(S, w, values)
    assert out.shape == (FULL, C)

    def refs():
        for k0, k1 in s.ray_chunks:                                    # rays k0 .. k1 - 1 own exactly samples k0 .. k1 - 1
            yield k0, k1, L.as_float32(L.ref_accumulate(w[k0:k1], values[k0:k1], S.ray[k0:k1].long() - k0, k1 - k0))
    assert_chunks_equal(out, refs(), "accumulate")
    lengths = S.counts
    for E in (L.E31, L.E32):                                           # the straddling rays are there, and not empty sums
        q = E // C - 100
        assert int(lengths[q]) == min(q + 200, FULL) - q and bool((out[q] != 0).any())
    assert int(lengths.max()) == L.LONG_RAY


@large(4 * HALF_BYTES + 3 * GIB)
def test_accumulate_backward(gpu):
    """grad_w [T] and grad_values [T, 1024] at 2^31 + 65536 elements (four arrays of 8 GiB are live in the backward)."""
    s = lists(HALF, gpu)
    S = s.samples
    values, w = filled(HALF, L.value_pattern, gpu).requires_grad_(True), weights_of(HALF, gpu).requires_grad_(True)
    g = filled(HALF, L.grad_pattern, gpu)
    L.assert_exact(C, L.GRAD_MAX * L.VALUE_MAX, "grad_w")
    L.assert_exact(1, L.WEIGHT_MAX * L.GRAD_MAX, "grad_values")
    out = svox.accumulate(S, w, values)
    out.backward(g)
    del out
    gv, gw = values.grad, w.grad
    assert gv.shape == (HALF, C) and gw.shape == (HALF,)
    wd, vd = w.detach(), values.detach()
    for k0, k1 in L.chunks(HALF, L.CHUNK_ROWS // 2):
        rw, rv = L.ref_accumulate_grads(wd[k0:k1], vd[k0:k1], S.ray[k0:k1], g)
        assert torch.equal(gw[k0:k1], L.as_float32(rw)), f"grad_w, samples {k0} .. {k1}"
        assert_chunks_equal(gv, [(k0, k1, rv)], "grad_values")
    assert bool((gw != 0).any()) and bool((gv[HALF - 64:] != 0).any())


# ------------------------------------------------------------------------------------------------------------- ray_scan
SCANS = [dict(exclusive=False, reverse=False), dict(exclusive=True, reverse=False), dict(exclusive=False, reverse=True)]


@large(2 * FULL_BYTES + 6 * GIB)
def test_ray_scan_forward(gpu):
    """sum, inclusive / exclusive / reverse, over values [2^22 + 64, 1024]: every row.  A ray of 2^17 samples, and rays
    across the rows that hold elements 2^31 and 2^32."""
    s = lists(FULL, gpu)
    values = filled(FULL, L.value_pattern, gpu)
    L.assert_exact(max(k1 - k0 for k0, k1 in s.ray_chunks), L.VALUE_MAX, "a chunk's running sum")
    for kw in SCANS:
        out = svox.ray_scan(s.samples, values, "sum", **kw)

        def refs():
            for k0, k1 in s.ray_chunks:
                start, end = s.segment(k0, k1)
                yield k0, k1, L.ref_segment_cumsum(values[k0:k1], start, end, **kw).to(torch.float32)
        assert_chunks_equal(out, refs(), f"ray_scan {kw}")
        q = L.E32 // C - 100                                              # the ray across element 2^32: its running sum moves
        assert bool((out[q + 99] != out[q + 101]).any())
        del out


@large(4 * HALF_BYTES + 4 * GIB)
def test_ray_scan_backward(gpu):
    """The gradient of the three sum scans at 2^31 + 65536 elements: the scan of the upstream gradient the other way."""
    s = lists(HALF, gpu)
    values = filled(HALF, L.value_pattern, gpu).requires_grad_(True)
    g = filled(HALF, L.grad_pattern, gpu)
    L.assert_exact(max(k1 - k0 for k0, k1 in s.ray_chunks), L.GRAD_MAX, "a chunk's running sum")
    for kw in SCANS:
        values.grad = None
        out = svox.ray_scan(s.samples, values, "sum", **kw)
        out.backward(g)
        del out

        def refs():
            for k0, k1 in s.ray_chunks:
                start, end = s.segment(k0, k1)
                yield k0, k1, L.ref_segment_cumsum(g[k0:k1], start, end, exclusive=kw["exclusive"], reverse=not kw["reverse"]).to(torch.float32)
        assert_chunks_equal(values.grad, refs(), f"ray_scan backward {kw}")


# ----------------------------------------------------------------------------------------------------------- optim_step
@large(2 * FULL_BYTES + 4 * GIB)
def test_feature_sgd_dense(gpu):
    """FeatureSGD(lazy=False), lr = 0.5, on an integer table of 2^32 + 65536 elements: p - g / 2 is exact."""
    p = filled(FULL, L.value_pattern, gpu).requires_grad_(True)
    p.grad = filled(FULL, L.grad_pattern, gpu)
    opt = svox.FeatureSGD([p], lr=0.5, lazy=False)
    opt.step()

    def refs():
        for k0, k1 in L.chunks(FULL, L.CHUNK_ROWS // 4):
            k = rows_of(k0, k1, gpu)
            want = L.value_pattern(k, C).double() - 0.5 * L.grad_pattern(k, C).double()
            yield k0, k1, want.to(torch.float32)
    assert_chunks_equal(p.detach(), refs(), "FeatureSGD")
    assert_chunks_equal(p.grad, ((k0, k1, L.grad_pattern(rows_of(k0, k1, gpu), C)) for k0, k1 in L.chunks(FULL)), "the gradient is read only", bits=True)


@large(4 * HALF_BYTES + 4 * GIB)
def test_feature_adam_lazy(gpu):
    """FeatureAdam(lazy=True) on four tables of 2^31 + 65536 elements: the gradient is non-zero in the window rows and in
    every 4099th row.  The touched rows equal tests/optim_restate.py bit for bit; every other row of the parameter and of
    both moments keeps its bits."""
    hp = dict(lr=0.25, betas=(0.9, 0.999), eps=1e-8)
    touched = L.sparse_grad_rows(HALF, C)
    td = torch.from_numpy(touched).to(gpu)
    p = filled(HALF, L.value_pattern, gpu).requires_grad_(True)
    m, v = filled(HALF, L.moment1_pattern, gpu), filled(HALF, L.moment2_pattern, gpu)
    g = torch.zeros((HALF, C), dtype=torch.float32, device=gpu)
    g[td] = L.grad_pattern(td, C)
    assert bool((g[td] != 0).any(dim=1).all())
    p.grad = g
    opt = svox.FeatureAdam([p], **hp)
    opt.state[p] = {"step": torch.tensor(2.0), "exp_avg": m, "exp_avg_sq": v}
    opt.step()
    assert opt.state[p]["exp_avg"] is m and opt.state[p]["exp_avg_sq"] is v and float(opt.state[p]["step"]) == 3.0
    # the touched rows, on the host
    tc = torch.from_numpy(touched)
    p0, g0, m0, v0 = (f(tc, C).numpy() for f in (L.value_pattern, L.grad_pattern, L.moment1_pattern, L.moment2_pattern))
    wp, wm, wv = OR.adam(p0, g0, m0, v0, 3, **hp)
    for name, got, want, old in (("p", p.detach(), wp, p0), ("exp_avg", m, wm, m0), ("exp_avg_sq", v, wv, v0)):
        np.testing.assert_array_equal(OR.bits(got[td].cpu().numpy()), OR.bits(want), err_msg=name)
        assert (OR.bits(want) != OR.bits(old)).any(axis=1).all(), name       # (every touched row moved: the comparison sees it)
    # every other row keeps its bits
    is_touched = torch.zeros(HALF, dtype=torch.bool, device=gpu)
    is_touched[td] = True
    for name, got, pattern in (("p", p.detach(), L.value_pattern), ("exp_avg", m, L.moment1_pattern), ("exp_avg_sq", v, L.moment2_pattern)):
        for k0, k1 in L.chunks(HALF):
            same = (got[k0:k1].view(torch.int32) == pattern(rows_of(k0, k1, gpu), C).view(torch.int32)).all(dim=1)
            wrong = torch.nonzero(~(same | is_touched[k0:k1]))
            assert wrong.numel() == 0, f"{name}: untouched row {k0 + int(wrong[0, 0])} changed"


# ---------------------------------------------------------------------------------------------------------- interp_rows
def stencil_of(Q, M, gpu):
    """A hand-made stencil: per point three corners with weights 0.5, 0.25 and 0.25 at hashed rows in [-1, M] (both ends are
    'no row'), the other five corners -1 with weight 0.  Which three corners: hashed too."""
    q = rows_of(0, Q, gpu)
    rows = torch.full((Q, 8), -1, dtype=torch.int32, device=gpu)
    weights = torch.zeros((Q, 8), dtype=torch.float32, device=gpu)
    first = L.mix(q) % 6
    for j, wj in enumerate((0.5, 0.25, 0.25)):
        corner = (first + j)[:, None]
        rows.scatter_(1, corner, (L.mix(q + (j + 1) * 7919) % (M + 2) - 1).to(torch.int32)[:, None])
        weights.scatter_(1, corner, torch.full((Q, 1), wj, dtype=torch.float32, device=gpu))
    return svox.InterpStencil(rows, weights)


@large(2 * FULL_BYTES + 5 * GIB)
def test_interp_rows(gpu):
    """interp_rows forward (out [2^22 + 64, 1024]: the vector kernel, and with a column permutation the scalar kernel is
    test_gather_rows' twin and is left to the small tests) and its table gradient, with a hand-made stencil whose weights
    are 0, 0.25 and 0.5 and an integer table: quarters of integers below 2^20, exact."""
    M = 1024
    st = stencil_of(FULL, M, gpu)
    table = L.table_pattern(rows_of(0, M, gpu), C).requires_grad_(True)          # below 2^20: a quarter of it has 22 bits
    out = svox.interp_rows(st, table)
    assert out.shape == (FULL, C)
    td = table.detach()

    def refs():
        for k0, k1 in L.chunks(FULL, L.CHUNK_ROWS // 2):
            acc = torch.zeros((k1 - k0, C), dtype=torch.float64, device=gpu)
            for j in range(8):
                r, wj = st.rows[k0:k1, j].long(), st.weights[k0:k1, j].double()
                ok = (r >= 0) & (r < M) & (wj != 0)
                if bool(ok.any()):
                    acc[ok] += wj[ok, None] * td[r[ok]].double()
            yield k0, k1, acc.to(torch.float32)
    assert_chunks_equal(out.detach(), refs(), "interp_rows")
    # the table gradient: sum over the entries e = 8 q + j of weights[e] * g[q, :], per row
    g = filled(FULL, L.grad_pattern, gpu)
    out.backward(g)
    del out
    want = torch.zeros((M, C), dtype=torch.float64, device=gpu)
    entries = torch.zeros((M,), dtype=torch.int64, device=gpu)
    for k0, k1 in L.chunks(FULL, L.CHUNK_ROWS // 2):
        for j in range(8):
            r, wj = st.rows[k0:k1, j].long(), st.weights[k0:k1, j]
            ok = (r >= 0) & (r < M) & (wj != 0)
            if bool(ok.any()):
                want.index_add_(0, r[ok], (wj[ok, None] * g[k0:k1][ok]).double())
                entries = L.ref_segment_count(r[ok], M, entries)
    # quarters: 4 |w g| <= 16 per entry, so four times the sum stays an integer below 2^24
    L.assert_exact(int(entries.max()), 4 * L.GRAD_MAX // 2, "interp_rows backward, in quarters")
    assert torch.equal(table.grad, want.to(torch.float32)), "the table gradient of interp_rows"
    assert bool((table.grad != 0).any(dim=1).all())


# ------------------------------------------------------------------------------- N3Tree.forward, its backward, N3Tree.set
def full_depth2_tree(K, features, gpu, rows=None):
    """A root whose eight slots are all refined once: 64 leaves of side 1 / 4; leaf l = 8 i + s (node 1 + i, slot s)
    names feature row l, or rows[l].  `features` may be a stand-in [1, K]: the calls below pass the table they mean."""
    child = np.zeros((9, 2, 2, 2), np.int32)
    child[0] = (1 + np.arange(8, dtype=np.int32)).reshape(2, 2, 2)                # the offset from node 0
    data = np.full((9, 2, 2, 2, 1), synth.EMPTY_SENTINEL, np.int32)
    data[1:] = (np.arange(64) if rows is None else np.asarray(rows)).astype(np.int32).reshape(8, 2, 2, 2, 1)
    pd = np.zeros((9, 2), np.int32)
    pd[1:, 0], pd[1:, 1] = np.arange(8), 1                                        # packed parent slot 0 * 8 + i, depth 1
    return svox.N3Tree.from_arrays(child, data, pd, features, data_format="RGBA", device=gpu)


def leaf_points(Q, gpu):
    """(points float32 [Q, 3], leaf int64 [Q]): window point q of window w lies in leaf 8 w + q % 8, every other point in
    one of the leaves 40 .. 55 (hashed); leaves 56 .. 63 receive nothing.  A hashed offset keeps the point inside its cell."""
    q = rows_of(0, Q, gpu)
    leaf = 40 + L.mix(q) % 16
    for w, (lo, hi) in reversed(list(enumerate(L.windows(Q, C)))):
        leaf = torch.where((q >= lo) & (q < hi), 8 * w + q % 8, leaf)
    i, s = leaf // 8, leaf % 8
    pts = []
    for a in (2, 1, 0):                                                           # x, y, z: the bits 4, 2, 1 of node and slot
        jitter = (L.mix(q + 1000003 * (a + 1)) % 1001).to(torch.float32) / 1000.0 * 0.2 + 0.025      # in [0.025, 0.225]
        pts.append(((i >> a) & 1).to(torch.float32) * 0.5 + ((s >> a) & 1).to(torch.float32) * 0.25 + jitter)
    return torch.stack(pts, dim=1).contiguous(), leaf


@large(2 * FULL_BYTES + 4 * GIB)
def test_point_query_backward_and_set(gpu):
    """N3Tree.forward at Q = 2^22 + 64 points and K = 1024 (values [Q, K]: 2^32 + 65536 elements), its backward (grad_out of
    that size) and N3Tree.set(reduce="last") from values of that size.  The row of every point comes from a twin tree of
    the same topology with K = 1 whose table holds the row number."""
    from tests import assign_restate as A
    Q, M = FULL, 72
    f = L.value_pattern(rows_of(0, M, gpu), C).requires_grad_(True)
    tree = full_depth2_tree(C, f.detach().cpu(), gpu)
    twin = full_depth2_tree(1, torch.arange(M, dtype=torch.float32)[:, None], gpu)
    points, leaf = leaf_points(Q, gpu)
    row = twin(twin.features.detach(), points)[:, 0].to(torch.int64)
    assert torch.equal(row, leaf), "the points do not lie in the leaves they were made for"
    count = L.ref_segment_count(row, M)
    assert bool((count[:56] > 0).all()) and not bool(count[56:].any())
    # forward: values == features[row], every point
    out = tree(f, points)
    assert out.shape == (Q, C)
    fd = f.detach()
    assert_chunks_equal(out.detach(), ((k0, k1, L.ref_gather(fd, row[k0:k1])) for k0, k1 in L.chunks(Q)), "N3Tree.forward", bits=True)
    # backward: float atomics over integers below 2^24 -- exact in any order
    g = filled(Q, L.grad_pattern, gpu)
    L.assert_exact(int(count.max()), L.GRAD_MAX, "the gradient of N3Tree.forward")
    out.backward(g)
    del out
    want = None
    for k0, k1 in L.chunks(Q, L.CHUNK_ROWS // 2):
        want = L.ref_segment_sum(g[k0:k1], row[k0:k1], M, want)
    assert torch.equal(f.grad, L.as_float32(want)), "the gradient of N3Tree.forward"
    assert bool((f.grad[:56] != 0).any(dim=1).all()) and not bool(f.grad[56:].any())
    # set(reduce="last"): every row with a point takes the values of its highest point, the others keep their bits
    table0 = L.value_pattern(rows_of(1000, 1000 + M, gpu), C)
    table = table0.clone()
    tree.set(points, g, reduce="last", features=table)
    rows_h = row.cpu().numpy()
    winner = np.full(M, -1, np.int64)
    np.maximum.at(winner, rows_h, np.arange(Q, dtype=np.int64))
    for w, (lo, hi) in enumerate(L.windows(Q, C)):                                # each window's leaves are won inside it
        assert ((winner[8 * w:8 * w + 8] >= lo) & (winner[8 * w:8 * w + 8] < hi)).all()
    pts = np.sort(winner[winner >= 0])
    want = A.assign_last(table0.cpu().numpy(), rows_h[pts], g[torch.from_numpy(pts).to(gpu)].cpu().numpy())
    np.testing.assert_array_equal(OR.bits(table.cpu().numpy()), OR.bits(want))
    assert (OR.bits(want[56:]) == OR.bits(table0[56:].cpu().numpy())).all() and (want[:56] != table0[:56].cpu().numpy()).any(axis=1).all()


@large(2 * FULL_BYTES + 5 * GIB)
def test_set_into_a_tall_table(gpu):
    """N3Tree.set, "last" and "sum", from values [2^22 + 64, 1024] into a table of 2^22 + 64 rows of 1024: the leaves name
    rows around the element boundaries of the TABLE, the launch is sized by min(Q, M) groups of 256 lanes (more than 2^30
    lanes).  Every row no leaf names keeps its bits."""
    Q = M = FULL
    win = L.window_rows(M, C)
    leaf_row = win[(np.arange(64) * 7) % win.shape[0]]                            # 64 distinct window rows (449 is a prime)
    assert np.unique(leaf_row).shape[0] == 64 and all(((leaf_row * C <= E) & (E < (leaf_row + 65) * C)).any() for E in L.BOUNDARIES)
    tree = full_depth2_tree(C, torch.zeros(1, C), gpu, rows=leaf_row)
    twin = full_depth2_tree(1, torch.zeros(1, 1), gpu, rows=leaf_row)
    points, leaf = leaf_points(Q, gpu)
    numbers = torch.arange(M, dtype=torch.float32, device=gpu)[:, None]           # (row numbers below 2^24: exact)
    row = twin(numbers, points)[:, 0].to(torch.int64)
    lr = torch.from_numpy(leaf_row).to(gpu)
    assert torch.equal(row, lr[leaf]), "the points do not lie in the leaves they were made for"
    del numbers
    values = filled(Q, L.grad_pattern, gpu)
    table = filled(M, L.value_pattern, gpu)
    named = lr[:56]                                                               # leaves 56 .. 63 receive no point

    def check(want_rows, what):
        def refs():
            for k0, k1 in L.chunks(M):
                want = L.value_pattern(rows_of(k0, k1, gpu), C)
                here = (named >= k0) & (named < k1)
                want[named[here] - k0] = want_rows[here]
                yield k0, k1, want
        assert_chunks_equal(table, refs(), what, bits=True)

    tree.set(points, values, reduce="last", features=table)
    winner = torch.full((64,), -1, dtype=torch.int64, device=gpu)
    winner.scatter_reduce_(0, leaf, rows_of(0, Q, gpu), "amax", include_self=True)
    assert bool((winner[:56] >= 0).all()) and bool((winner[56:] < 0).all())
    check(values[winner[:56]], 'set(reduce="last")')
    count = L.ref_segment_count(leaf, 64)
    L.assert_exact(int(count.max()), L.GRAD_MAX, 'set(reduce="sum")')
    total = None
    for k0, k1 in L.chunks(Q, L.CHUNK_ROWS // 2):
        total = L.ref_segment_sum(values[k0:k1], leaf[k0:k1], 64, total)
    tree.set(points, values, reduce="sum", features=table)
    check(L.as_float32(total)[:56], 'set(reduce="sum")')


@large(FULL_BYTES + 3 * GIB)
def test_reduce_rows_into_a_tall_table(gpu):
    """reduce_rows with M = 2^22 + 64 rows of 1024: out has 2^32 + 65536 elements and a lane each (the short rows' kernel);
    three samples name each window row of `out`, the rest of it is `empty`."""
    M = FULL
    win = L.window_rows(M, C)
    n = win.shape[0]
    row = torch.from_numpy(np.concatenate([np.tile(win, 3), [-1, M, -1, M]]).astype(np.int32)).to(gpu)
    T = row.shape[0]
    z = torch.zeros(T, dtype=torch.float32, device=gpu)
    S = svox.RaySamples(torch.tensor([0, T], dtype=torch.int64, device=gpu), torch.zeros(T, dtype=torch.int32, device=gpu), row, z, z + 1)
    values = L.value_pattern(rows_of(0, T, gpu), C)
    wd = torch.from_numpy(win).to(gpu)
    three = values[:3 * n].reshape(3, n, C)
    for op, empty, want_rows in (("sum", -7.0, three.double().sum(0).to(torch.float32)), ("max", 5.5, three.amax(0))):
        out = svox.reduce_rows(S, values, M, op, empty=empty)
        assert out.shape == (M, C)

        def refs():
            for k0, k1 in L.chunks(M):
                want = torch.full((k1 - k0, C), empty, dtype=torch.float32, device=gpu)
                here = (wd >= k0) & (wd < k1)
                want[wd[here] - k0] = want_rows[here]
                yield k0, k1, want
        assert_chunks_equal(out, refs(), f"reduce_rows {op}", bits=True)
        del out


# -------------------------------------------------------------------------------------------------------- shade_samples
def shade_setup(T, gpu, aligned=True):
    """RGBA lists of T samples over a [2048, 1024] table: window sample i names row i % 97, every other sample a hashed row
    of 512 .. 2047 or none (-1, M).  Returns (samples, row, features, renderer, window rows numpy, on the device)."""
    M, K, RES = 2048, C, 512
    k = rows_of(0, T, gpu)
    win = L.window_rows(T, K)
    wd = torch.from_numpy(win).to(gpu)
    r = L.mix(k) % (M - RES + 2)
    row = torch.where(r == 0, torch.full_like(r, -1), RES - 1 + r)                # -1, or RES .. M (M: outside too)
    row[wd] = torch.arange(win.shape[0], dtype=torch.int64, device=gpu) % 97
    row = row.to(torch.int32)
    assert int(row.min()) == -1 and int(row.max()) == M
    z = torch.zeros(T, dtype=torch.float32, device=gpu)
    samples = svox.RaySamples(torch.tensor([0, T], dtype=torch.int64, device=gpu), torch.zeros(T, dtype=torch.int32, device=gpu), row, z, z + 1)
    flat = torch.empty(M * K + 4, dtype=torch.float32, device=gpu)
    f = flat[0 if aligned else 1:][:M * K].view(M, K)
    f.copy_((((L.mix(rows_of(0, M * K, gpu)) % 2001) - 1000).to(torch.float32) / 250.0).reshape(M, K))
    assert (f.data_ptr() % 16 == 0) == aligned and f.is_contiguous()
    tree = svox.N3Tree(N=2, data_dim=K, data_format="RGBA", map_location=gpu)
    return samples, row, f, svox.VolumeRenderer(tree), win, wd


def shade_forward_checks(gpu, samples, row, f, rend, win, wd, values, sigma):
    """The window samples against tests/shade_restate.py, every chunk against the operator on that chunk alone; returns
    (opt, features on the host, the window samples' rows, rays and restated values)."""
    from oracle import oracle as O
    from tests import shade_restate as SR
    T, K = row.shape[0], f.shape[1]
    assert values.shape == (T, K - 1) and sigma.shape == (T,)
    df = svox.DataFormat("RGBA")
    opt = O.make_options(format=df.format, basis_dim=df.basis_dim)
    feats, row_w = f.detach().cpu().numpy(), row[wd].cpu().numpy()
    ray_w = np.zeros(win.shape[0], np.int64)
    want_v, want_s = SR.forward(feats, row_w, ray_w, opt, None, True)
    np.testing.assert_array_equal(OR.bits(values[wd].detach().cpu().numpy()), OR.bits(want_v))
    np.testing.assert_array_equal(OR.bits(sigma[wd].detach().cpu().numpy()), OR.bits(want_s))
    fd = f.detach()
    z = torch.zeros(L.CHUNK_ROWS, dtype=torch.float32, device=gpu)
    for k0, k1 in L.chunks(T):
        n = k1 - k0
        sub = svox.RaySamples(torch.tensor([0, n], dtype=torch.int64, device=gpu), torch.zeros(n, dtype=torch.int32, device=gpu),
                              row[k0:k1].contiguous(), z[:n], z[:n] + 1)
        v2, s2 = rend.shade_samples(sub, fd)
        assert torch.equal(values[k0:k1].detach().view(torch.int32), v2.view(torch.int32)), f"values, samples {k0} .. {k1}"
        assert torch.equal(sigma[k0:k1].detach().view(torch.int32), s2.view(torch.int32)), f"sigma, samples {k0} .. {k1}"
        del v2, s2
    return opt, feats, row_w, ray_w, want_v


@large(2 * HALF_BYTES + 4 * GIB)
def test_shade_samples_rgba(gpu):
    """RGBA, K = 1024: values [T, 1023] and sigma with T (C + 1) = 2^31 + 65536.  The window samples equal
    tests/shade_restate.py bit for bit; every chunk equals, bit for bit, the same operator on that chunk's samples alone
    (which the small tests pin).  The table gradient equals the restatement on the rows the window samples name: rows
    0 .. 96, which no other sample names."""
    from tests import shade_restate as SR
    T, K, RES = HALF, C, 512
    samples, row, f, rend, win, wd = shade_setup(T, gpu)
    f.requires_grad_(True)
    values, sigma = rend.shade_samples(samples, f)
    opt, feats, row_w, ray_w, want_v = shade_forward_checks(gpu, samples, row, f, rend, win, wd, values, sigma)
    # the table gradient
    gv = torch.empty((T, K - 1), dtype=torch.float32, device=gpu)
    for k0, k1 in L.chunks(T):
        gv[k0:k1] = L.grad_pattern(rows_of(k0, k1, gpu), K - 1)
    gs = (rows_of(0, T, gpu) % 7 - 3).to(torch.float32)
    grad = torch.autograd.grad([values, sigma], [f], [gv, gs])[0]
    want = SR.grad(feats, row_w, ray_w, opt, None, want_v, gv[wd].cpu().numpy(), gs[wd].cpu().numpy(), True)
    np.testing.assert_array_equal(OR.bits(grad[:97].cpu().numpy()), OR.bits(want[:97]))
    assert (want[:97] != 0).any(axis=1).all() and not bool(grad[97:RES].any()) and bool((grad[RES:] != 0).any(dim=1).all())


@pytest.mark.parametrize("kernel", ["float4", "scalar"])
@large(FULL_BYTES + 3 * GIB)
def test_shade_samples_rgba_forward_full(gpu, kernel):
    """The forward alone at T = 2^22 + 64 (values: 2^32 elements less 2^22 + 64, past all three boundaries), where a launch
    of a lane per element no longer fits 32 bits: the 16-byte kernel (2^30 + 16384 lanes) and, with a table that does not
    start on a 16-byte line, the scalar one (2^32 + 65536 lanes)."""
    samples, row, f, rend, win, wd = shade_setup(FULL, gpu, aligned=kernel == "float4")
    values, sigma = rend.shade_samples(samples, f)
    shade_forward_checks(gpu, samples, row, f, rend, win, wd, values, sigma)


@pytest.mark.parametrize("fmt,K", [("SH1", 1024), ("SH4", 1025)])
@large(FULL_BYTES + 3 * GIB)
def test_shade_samples_rotated_forward_full(gpu, fmt, K):
    """shade_samples(rotations=), the forward, at T = 2^22 + 64 samples: SH1 with K = 1024 has C + 1 = 1024 lanes a sample
    (2^32 + 65536 lanes, values of 2^32 elements less T), SH4 with K = 1025 has 257 (2^30 + 2^22 and some lanes: the grid
    folds, and the basis does depend on the rotated direction).  The window samples equal tests/viewrot_restate.py bit
    for bit; every chunk equals, bit for bit, the operator on that chunk's samples alone.  Rows and rays outside their
    ranges occur."""
    from oracle import oracle as O
    from tests import viewrot_restate as VR
    T, M, Q = FULL, 512, 257
    k = rows_of(0, T, gpu)
    row = (L.mix(k) % (M + 2) - 1).to(torch.int32)
    ray = (L.mix(k + 7919) % (Q + 2) - 1).to(torch.int32)
    assert int(row.min()) == -1 and int(row.max()) == M and int(ray.min()) == -1 and int(ray.max()) == Q
    z = torch.zeros(L.CHUNK_ROWS, dtype=torch.float32, device=gpu)

    def lists_of(k0, k1):
        n = k1 - k0
        offsets = torch.full((Q + 1,), n, dtype=torch.int64, device=gpu)
        offsets[0] = 0
        depth = torch.zeros(n, dtype=torch.float32, device=gpu) if n > z.shape[0] else z[:n]
        return svox.RaySamples(offsets, ray[k0:k1].contiguous(), row[k0:k1].contiguous(), depth, depth + 1)

    f = (((L.mix(rows_of(0, M * K, gpu)) % 2001) - 1000).to(torch.float32) / 250.0).reshape(M, K)
    rot = (((L.mix(rows_of(0, M * 9, gpu) + 104729) % 2001) - 1000).to(torch.float32) / 1000.0).reshape(M, 3, 3)
    v = ((L.mix(rows_of(0, Q * 3, gpu) + 1299709) % 2001) - 1000).to(torch.float32) + 0.5
    v = torch.nn.functional.normalize(v.reshape(Q, 3), dim=1).contiguous()
    rays = svox.Rays(torch.zeros_like(v), v.clone(), v)
    tree = svox.N3Tree(N=2, data_dim=K, data_format=fmt, map_location=gpu)
    rend = svox.VolumeRenderer(tree)
    with torch.no_grad():
        values, sigma = rend.shade_samples(lists_of(0, T), f, rays, rotations=rot)
    df = svox.DataFormat(fmt)
    C = (K - 1) // df.basis_dim
    assert values.shape == (T, C) and sigma.shape == (T,) and T * (C + 1) > 2 ** 30
    opt = O.make_options(format=df.format, basis_dim=df.basis_dim)
    win = L.window_rows(T, C)
    wd = torch.from_numpy(win).to(gpu)
    want_v, want_s = VR.forward32(f.cpu().numpy(), row[wd].cpu().numpy(), ray[wd].cpu().numpy(), opt, rot.cpu().numpy(), v.cpu().numpy(), None, True)
    np.testing.assert_array_equal(OR.bits(values[wd].cpu().numpy()), OR.bits(want_v))
    np.testing.assert_array_equal(OR.bits(sigma[wd].cpu().numpy()), OR.bits(want_s))
    assert (want_v != 0).any() and (want_v == 0).all(axis=1).any()
    with torch.no_grad():
        for k0, k1 in L.chunks(T):
            v2, s2 = rend.shade_samples(lists_of(k0, k1), f, rays, rotations=rot)
            assert torch.equal(values[k0:k1].view(torch.int32), v2.view(torch.int32)), f"values, samples {k0} .. {k1}"
            assert torch.equal(sigma[k0:k1].view(torch.int32), s2.view(torch.int32)), f"sigma, samples {k0} .. {k1}"
            del v2, s2


# -------------------------------------------------------------------------------------------------------------- tv_rows
@large(2 * HALF_BYTES + 3 * GIB)
def test_tv_rows(gpu):
    """tv_rows, loss and gradient, p = 2, over features [2^21 + 64, 1024] (2^31 + 65536 elements: a lane per element) with a
    hand-made edge plan: 64 edges across the row of element 2^30, 64 across the row of element 2^31, 64 from the first rows
    to the last.  Integer features: the loss and the gradient are exact."""
    from svox_t_amd import csrc as _C
    M = HALF
    f = filled(M, L.small_pattern, gpu)
    i = np.arange(64, dtype=np.int64)
    a = np.concatenate([L.E30 // C - 1 - i, L.E31 // C - 1 - i, i])
    b = np.concatenate([L.E30 // C + i, L.E31 // C + i, M - 1 - i])
    E = a.shape[0]
    assert (a < b).all() and b.max() == M - 1 and E == 192
    L.assert_exact(E * C, 6 * 6, "the tv loss")
    # the CSR over rows: each edge once from its lower row (meta 0: this entry carries the loss) and once from its upper (1)
    rows = np.concatenate([a, b])
    order = np.argsort(rows, kind="stable")
    other = np.concatenate([b, a])[order].astype(np.int32)
    meta = np.concatenate([np.zeros(E, np.uint8), np.ones(E, np.uint8)])[order]
    row_ptr = np.searchsorted(rows[order], np.arange(M + 1), side="left").astype(np.int32)
    plan = _C._extras.TVPlan(torch.from_numpy(row_ptr).to(gpu), torch.from_numpy(other).to(gpu), torch.from_numpy(meta).to(gpu), E, M,
                             torch.ones(32, dtype=torch.float32, device=gpu))
    loss, G = _C._extras.tv_rows(f, plan, None, 2, "uniform", False, "loss_grad")
    touched = np.unique(rows)
    td = torch.from_numpy(touched).to(gpu)
    fh = dict(zip(touched.tolist(), f[td].cpu().numpy().astype(np.int64)))
    want_loss, want_G = 0, {r: np.zeros(C, np.int64) for r in touched.tolist()}
    for x, y in zip(a.tolist(), b.tolist()):
        d = fh[x] - fh[y]
        want_loss += int((d * d).sum())
        want_G[x] += 2 * d
        want_G[y] -= 2 * d
    assert 0 < want_loss < L.EXACT and float(loss) == float(want_loss)
    np.testing.assert_array_equal(G[td].cpu().numpy(), np.stack([want_G[r] for r in touched.tolist()]).astype(np.float32))
    assert bool((G[td] != 0).any())
    untouched = torch.ones(M, dtype=torch.bool, device=gpu)
    untouched[td] = False
    for k0, k1 in L.chunks(M):
        wrong = torch.nonzero((G[k0:k1] != 0).any(dim=1) & untouched[k0:k1])
        assert wrong.numel() == 0, f"G: row {k0 + int(wrong[0, 0])} has no edge and is not zero"


@large(FULL_BYTES + 10 * GIB)
def test_interp_rows_many_points(gpu):
    """interp_rows forward at Q = 2^26 + 64 points of K = 64 columns: out has 2^32 + 4096 elements, and 16 lanes a point
    make 2^30 + 1024 lanes."""
    K, Q, M = 64, 2 ** 26 + 64, 1024
    st = stencil_of(Q, M, gpu)
    table = L.table_pattern(rows_of(0, M, gpu), K)
    out = svox.interp_rows(st, table)
    assert out.shape == (Q, K) and Q * K > L.E32

    def refs():
        for k0, k1 in L.chunks(Q, 2 ** 21):
            acc = torch.zeros((k1 - k0, K), dtype=torch.float64, device=gpu)
            for j in range(8):
                r, wj = st.rows[k0:k1, j].long(), st.weights[k0:k1, j].double()
                ok = (r >= 0) & (r < M) & (wj != 0)
                if bool(ok.any()):
                    acc[ok] += wj[ok, None] * table[r[ok]].double()
            yield k0, k1, acc.to(torch.float32)
    assert_chunks_equal(out, refs(), "interp_rows, many points")
    assert bool((out[L.E32 // K - 64:L.E32 // K + 64] != 0).any())


@large(16 * GIB)
def test_ray_quantile_many_quantiles(gpu):
    """ray_quantile with Q = 2^20 + 64 rays and 1024 quantiles: index and frac have 2^30 + 65536 elements and a lane each.
    The rays around the element boundaries hold five samples each and equal tests/scan_restate.py; every other ray is
    empty: index -1, frac 0."""
    from tests import scan_restate as SC
    Q, nq, per = 2 ** 20 + 64, 1024, 5
    rays = L.window_rows(Q, nq)
    T = per * rays.shape[0]
    counts = np.zeros(Q, np.int64)
    counts[rays] = per
    offsets_h = np.concatenate([[0], np.cumsum(counts)])
    w = L.weight_pattern(rows_of(0, T, gpu)) * 0.5                                # 0 (passed over), 0.5 and 1
    z = torch.zeros(T, dtype=torch.float32, device=gpu)
    ray = torch.from_numpy(np.repeat(rays, per).astype(np.int32)).to(gpu)
    S = svox.RaySamples(torch.from_numpy(offsets_h).to(gpu), ray, torch.zeros(T, dtype=torch.int32, device=gpu), z, z + 1)
    qs = torch.linspace(0, 1, nq)
    index, frac = svox.ray_quantile(S, w, qs)
    assert index.shape == (Q, nq) == frac.shape
    want_i, want_f = SC.quantile(w.cpu().numpy(), np.concatenate([offsets_h[rays], [T]]), qs.numpy(), True)
    rd = torch.from_numpy(rays).to(gpu)
    np.testing.assert_array_equal(index[rd].cpu().numpy(), want_i)
    np.testing.assert_array_equal(OR.bits(frac[rd].cpu().numpy()), OR.bits(want_f))
    assert (want_i >= 0).any() and (want_f > 0).any()
    empty = torch.ones(Q, dtype=torch.bool, device=gpu)
    empty[rd] = False
    for k0, k1 in L.chunks(Q, 2 ** 17):
        wrong = torch.nonzero(((index[k0:k1] != -1) | (frac[k0:k1] != 0)).any(dim=1) & empty[k0:k1])
        assert wrong.numel() == 0, f"ray {k0 + int(wrong[0, 0])} has no sample and is not (-1, 0)"
