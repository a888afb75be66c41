"""ray_scan, ray_quantile and RaySamples.select without a GPU: the C ABI's argument checks, the Python layer's, and the
restatement (tests/scan_restate.py) against its own float64 autograd and against the lists' restatement."""
import ctypes

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from tests import samples_restate as R
from tests import scan_restate as S
from tests.util import Case

NAMES = ("svoxt_ray_scan_fwd", "svoxt_ray_scan_bwd", "svoxt_ray_quantile", "svoxt_samples_select_workspace_bytes",
         "svoxt_samples_select_count", "svoxt_samples_select_emit")


def test_symbols_and_abi_version():
    lib = ctypes.CDLL(_C.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _C.EXPORTS
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22
    for name in ("ray_scan", "ray_quantile", "quantile_depth"):
        assert callable(getattr(svox, name)) and name in svox.__all__
    assert callable(svox.RaySamples.select)
    wb = _C._lib.svoxt_samples_select_workspace_bytes
    assert wb(0) == 0 and wb(-1) == -1 and wb(1 << 31) == -1
    assert wb(1) > 0 and wb(1) % 256 == 0 and wb(100000) >= 2 * 4 * 100001
    assert _C._extras.SCAN_OPS == {"sum": 0, "prod": 1, "max": 2, "min": 3}


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _C._lib
    err = lib.svoxt_last_error
    buf = (ctypes.c_float * 160)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    p2 = ctypes.c_void_p(p.value + 256)                # a second array: 4 * T * C = 48 bytes and more away from p
    p3 = ctypes.c_void_p(p.value + 384)
    odd4 = ctypes.c_void_p(p.value + 4)                # 4-byte aligned, not 8
    odd1 = ctypes.c_void_p(p3.value + 1)
    sf, sb, qt = lib.svoxt_ray_scan_fwd, lib.svoxt_ray_scan_bwd, lib.svoxt_ray_quantile
    cnt, emit = lib.svoxt_samples_select_count, lib.svoxt_samples_select_emit

    # extents
    for Q, Tn in ((-1, 4), (1 << 31, 4), (4, -1), (4, 1 << 31)):
        assert sf(p, Q, Tn, p, 1, 0, 0, p2, None) == 1 and b"svoxt_ray_scan_fwd: " in err() and b"must be in [0, 2^31)" in err()
        assert sb(p, Q, Tn, p, 1, 0, 0, p2, p3, None) == 1 and b"svoxt_ray_scan_bwd: " in err() and b"must be in [0, 2^31)" in err()
        assert qt(p, Q, Tn, p, p, 1, 1, p2, p3, None) == 1 and b"svoxt_ray_quantile: " in err() and b"must be in [0, 2^31)" in err()
        assert cnt(p, p, Q, Tn, p2, p3, p, 1 << 20, None) == 1 and b"svoxt_samples_select_count: " in err() and b"must be in [0, 2^31)" in err()
    for Tn in (-1, 1 << 31):
        assert emit(p, Tn, p, 1 << 20, p, p, p, p, 1, p2, p2, p2, p2, p2, None) == 1 and b"svoxt_samples_select_emit: T must be" in err()
    for To in (-1, 5):
        assert emit(p, 4, p, 1 << 20, p, p, p, p, To, p2, p2, p2, p2, p2, None) == 1 and b"svoxt_samples_select_emit: T_out must be in [0, T]" in err()
    # C, op, flags, nq
    for C in (0, -3):
        assert sf(p, 4, 4, p, C, 0, 0, p2, None) == 1 and b"svoxt_ray_scan_fwd: C must be >= 1" in err()
        assert sb(p, 4, 4, p, C, 0, 0, p2, p3, None) == 1 and b"svoxt_ray_scan_bwd: C must be >= 1" in err()
    for op in (-1, 4):
        assert sf(p, 4, 4, p, 1, op, 0, p2, None) == 1 and b"svoxt_ray_scan_fwd: op must be" in err()
        assert sb(p, 4, 4, p, 1, op, 0, p2, p3, None) == 1 and b"svoxt_ray_scan_bwd: op must be" in err()
    for flags in (-1, 4):
        assert sf(p, 4, 4, p, 1, 0, flags, p2, None) == 1 and b"svoxt_ray_scan_fwd: flags must be" in err()
        assert sb(p, 4, 4, p, 1, 0, flags, p2, p3, None) == 1 and b"svoxt_ray_scan_bwd: flags must be" in err()
    for nq in (0, -2):
        assert qt(p, 4, 4, p, p, nq, 1, p2, p3, None) == 1 and b"svoxt_ray_quantile: nq must be >= 1" in err()
    # NULLs
    assert sf(None, 4, 4, p, 1, 0, 0, p2, None) == 1 and b"svoxt_ray_scan_fwd: offsets is NULL" in err()
    assert sf(p, 4, 4, None, 1, 0, 0, p2, None) == 1 and b"svoxt_ray_scan_fwd: values / out is NULL" in err()
    assert sf(p, 4, 4, p, 1, 0, 0, None, None) == 1 and b"svoxt_ray_scan_fwd: values / out is NULL" in err()
    assert sb(None, 4, 4, p, 1, 0, 0, p2, p3, None) == 1 and b"svoxt_ray_scan_bwd: offsets is NULL" in err()
    assert sb(p, 4, 4, p, 1, 0, 0, None, p3, None) == 1 and b"svoxt_ray_scan_bwd: grad_out / grad_values is NULL" in err()
    assert sb(p, 4, 4, p, 1, 0, 0, p2, None, None) == 1 and b"svoxt_ray_scan_bwd: grad_out / grad_values is NULL" in err()
    for op in (1, 2, 3):
        assert sb(p, 4, 4, None, 1, op, 0, p2, p3, None) == 1 and b"svoxt_ray_scan_bwd: values is NULL" in err()
    assert qt(None, 4, 4, p, p, 1, 1, p2, p3, None) == 1 and b"svoxt_ray_quantile: offsets / q is NULL" in err()
    assert qt(p, 4, 4, p, None, 1, 1, p2, p3, None) == 1 and b"svoxt_ray_quantile: offsets / q is NULL" in err()
    assert qt(p, 4, 4, None, p, 1, 1, p2, p3, None) == 1 and b"svoxt_ray_quantile: w is NULL" in err()
    assert qt(p, 4, 4, p, p, 1, 1, None, p3, None) == 1 and b"svoxt_ray_quantile: index / frac is NULL" in err()
    assert qt(p, 4, 4, p, p, 1, 1, p2, None, None) == 1 and b"svoxt_ray_quantile: index / frac is NULL" in err()
    need = lib.svoxt_samples_select_workspace_bytes(4)
    assert cnt(p, p, 4, 4, None, p3, p, need, None) == 1 and b"svoxt_samples_select_count: offsets_out / total is NULL" in err()
    assert cnt(p, p, 4, 4, p2, None, p, need, None) == 1 and b"svoxt_samples_select_count: offsets_out / total is NULL" in err()
    assert cnt(None, p, 4, 4, p2, p3, p, need, None) == 1 and b"svoxt_samples_select_count: keep / offsets is NULL" in err()
    assert cnt(p, None, 4, 4, p2, p3, p, need, None) == 1 and b"svoxt_samples_select_count: keep / offsets is NULL" in err()
    assert cnt(p, p, 4, 4, p2, p3, None, need, None) == 1 and b"svoxt_samples_select_count: workspace is NULL" in err()
    assert cnt(p, p, 4, 4, p2, p3, p, need - 1, None) == 1 and b"svoxt_samples_select_count: workspace smaller" in err()
    assert emit(None, 4, p, need, p, p, p, p, 2, p2, p2, p2, p2, p2, None) == 1 and b"svoxt_samples_select_emit: keep is NULL" in err()
    for a in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert emit(p, 4, p, need, *a, 2, p2, p2, p2, p2, p2, None) == 1 and b"svoxt_samples_select_emit: ray / row / depth / length is NULL" in err()
    for i in range(5):
        outs = [p2] * 5
        outs[i] = None
        assert emit(p, 4, p, need, p, p, p, p, 2, *outs, None) == 1 and b"svoxt_samples_select_emit: an output is NULL" in err()
    assert emit(p, 4, None, need, p, p, p, p, 2, p2, p2, p2, p2, p2, None) == 1 and b"svoxt_samples_select_emit: workspace is NULL" in err()
    assert emit(p, 4, p, need - 1, p, p, p, p, 2, p2, p2, p2, p2, p2, None) == 1 and b"svoxt_samples_select_emit: workspace smaller" in err()
    # alignment: 8 bytes for the int64 arrays and the workspace, 4 for float32 / int32; keep is bytes
    for a in ((odd4, p, p2), (p, odd1, p2), (p, p, odd1)):
        assert sf(a[0], 4, 4, a[1], 1, 0, 0, a[2], None) == 1 and b"svoxt_ray_scan_fwd: a misaligned argument" in err()
    for a in ((odd4, p, p2, p3), (p, odd1, p2, p), (p, p, odd1, p3), (p, p, p2, odd1)):
        assert sb(a[0], 4, 4, a[1], 1, 1, 0, a[2], a[3], None) == 1 and b"svoxt_ray_scan_bwd: a misaligned argument" in err()
    for a in ((odd4, p, p, p2, p3), (p, odd1, p, p2, p3), (p, p, odd1, p2, p3), (p, p, p, odd4, p3), (p, p, p, p2, odd1)):
        assert qt(a[0], 4, 4, a[1], a[2], 1, 1, a[3], a[4], None) == 1 and b"svoxt_ray_quantile: a misaligned argument" in err()
    assert cnt(odd1, odd4, 4, 4, p2, p3, p, need, None) == 1 and b"svoxt_samples_select_count: offsets is not 8-byte aligned" in err()
    assert cnt(odd1, p, 4, 4, odd4, p3, p, need, None) == 1 and b"svoxt_samples_select_count: offsets_out / total is not 8-byte" in err()
    assert cnt(odd1, p, 4, 4, p2, odd4, p, need, None) == 1 and b"svoxt_samples_select_count: offsets_out / total is not 8-byte" in err()
    assert cnt(odd1, p, 4, 4, p2, p3, odd4, need, None) == 1 and b"svoxt_samples_select_count: workspace is not 8-byte aligned" in err()
    for i in range(4):
        ins = [p] * 4
        ins[i] = odd1
        assert emit(odd1, 4, p, need, *ins, 2, p2, p2, p2, p2, p2, None) == 1 and b"svoxt_samples_select_emit: a misaligned argument" in err()
    for i in range(5):
        outs = [p2] * 5
        outs[i] = odd1 if i < 4 else odd4
        assert emit(odd1, 4, p, need, p, p, p, p, 2, *outs, None) == 1 and b"svoxt_samples_select_emit: a misaligned argument" in err()
    assert emit(odd1, 4, odd4, need, p, p, p, p, 2, p2, p2, p2, p2, p2, None) == 1 and b"svoxt_samples_select_emit: workspace is not 8-byte aligned" in err()
    # aliasing: the scan reads values behind what it has written only by its own lane's order -- out must be another array
    assert sf(p, 4, 4, p2, 3, 0, 0, p2, None) == 1 and b"svoxt_ray_scan_fwd: out overlaps values" in err()
    assert sf(p, 4, 4, p2, 3, 0, 0, ctypes.c_void_p(p2.value + 44), None) == 1 and b"svoxt_ray_scan_fwd: out overlaps values" in err()
    assert sb(p, 4, 4, p, 3, 1, 0, p2, p2, None) == 1 and b"svoxt_ray_scan_bwd: grad_values overlaps" in err()
    assert sb(p, 4, 4, p2, 3, 1, 0, p3, p2, None) == 1 and b"svoxt_ray_scan_bwd: grad_values overlaps" in err()
    assert cnt(odd1, p, 4, 4, p, p3, p, need, None) == 1 and b"svoxt_samples_select_count: offsets_out overlaps offsets" in err()

    # Q = 0 / T = 0 are valid no-ops
    assert sf(None, 0, 0, None, 1, 0, 0, None, None) == 0 and sf(None, 0, 4, None, 2, 3, 3, None, None) == 0
    assert sf(None, 4, 0, None, 1, 1, 1, None, None) == 0
    assert sb(None, 0, 0, None, 1, 0, 0, None, None, None) == 0 and sb(None, 4, 0, None, 1, 2, 0, None, None, None) == 0
    assert qt(None, 0, 0, None, None, 1, 1, None, None, None) == 0 and qt(None, 0, 4, None, None, 3, 0, None, None, None) == 0
    assert emit(None, 0, None, 0, None, None, None, None, 0, None, None, None, None, None, None) == 0
    assert emit(None, 4, None, 0, None, None, None, None, 0, None, None, None, None, None, None) == 0


def cpu_samples(T=6):
    off = torch.tensor([0, 2, 2, T], dtype=torch.int64)
    return svox.RaySamples(off, torch.zeros(T, dtype=torch.int32), torch.zeros(T, dtype=torch.int32), torch.zeros(T), torch.ones(T))


def test_python_layer_checks_device_shapes_and_dtypes():
    s = cpu_samples()
    for kw in (dict(), dict(op="prod", exclusive=True), dict(op="max", reverse=True)):
        with pytest.raises(RuntimeError, match="GPU"):
            svox.ray_scan(s, torch.ones(6), **kw)
        with pytest.raises(RuntimeError, match="GPU"):
            svox.ray_scan(s, torch.ones(6, 3), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        svox.ray_quantile(s, torch.ones(6), [0.5])
    with pytest.raises(RuntimeError, match="GPU"):
        svox.quantile_depth(s, torch.ones(6), 0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        s.select(torch.ones(6, dtype=torch.bool))
    for v in (torch.ones(5), torch.ones(7, 2), torch.ones(6, 2, 1), torch.ones(6, 0), torch.ones(6, dtype=torch.float64),
              torch.ones(6, 2, dtype=torch.int32), None):
        with pytest.raises(RuntimeError, match=r"values must be float32 \[T\] or \[T, C\]"):
            svox.ray_scan(s, v)
    for op in ("mean", "cumsum", None, 0):
        with pytest.raises(RuntimeError, match="op must be one of"):
            svox.ray_scan(s, torch.ones(6), op)
    with pytest.raises(RuntimeError, match="samples must be a RaySamples"):
        svox.ray_scan((s.offsets,), torch.ones(6))
    with pytest.raises(RuntimeError, match="samples must be a RaySamples"):
        svox.ray_quantile((s.offsets,), torch.ones(6), [0.5])
    for w in (torch.ones(5), torch.ones(6, 1), torch.ones(6, dtype=torch.float64), None):
        with pytest.raises(RuntimeError, match=r"w must be float32 \[T\]"):
            svox.ray_quantile(s, w, [0.5])
    for q in ([], [1.5], [-0.1, 0.5], [float("nan")], torch.tensor([0.5], dtype=torch.float64), torch.ones(2, 2), "half", None,
              torch.tensor([0.2, 1.0001])):
        with pytest.raises(RuntimeError, match="ray_quantile: q must"):
            svox.ray_quantile(s, torch.ones(6), q)
    for keep in (torch.ones(5, dtype=torch.bool), torch.ones(6, dtype=torch.uint8), torch.ones(6), torch.ones(6, 1, dtype=torch.bool),
                 [True] * 6, None):
        with pytest.raises(RuntimeError, match=r"keep must be torch.bool \[T\]"):
            s.select(keep)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C._extras.ray_scan(s.offsets, torch.ones(6, 1))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _C._extras.samples_select(torch.ones(6, dtype=torch.bool), s.offsets, s.ray, s.row, s.depth, s.length)


# ------------------------------------------------------------------------------------------------- the restatement
LENGTHS = (0, 1, 2, 17, 40, 0, 33, 5)                  # the longest ray of the fixture: n = 40


def fixture(op, seed, C=2):
    rng = np.random.default_rng(seed)
    counts = np.array(LENGTHS * 2)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    T = int(offsets[-1])
    if op == "prod":
        v = rng.uniform(0.25, 1.0, (T, C)).astype(np.float32)
        v[rng.choice(T, 6, replace=False), rng.integers(0, C, 6)] = 0.0              # a few exact zeros
        v[int(offsets[4]) + 7, 0] = 0.0                                               # ... one of them inside the longest ray
    else:
        v = rng.standard_normal((T, C)).astype(np.float32)
        if op in ("max", "min"):
            v[::9] = v[3::9][: v[::9].shape[0]]                                       # ties
    g = rng.standard_normal((T, C)).astype(np.float32)
    return offsets, v, g


def test_restated_forward_is_the_plain_loop():
    """The position-by-position form against the most literal one: a Python loop per ray and channel in np.float32."""
    for op in S.OPS:
        offsets, v, _ = fixture(op, 3)
        for exclusive in (False, True):
            for reverse in (False, True):
                got = S.scan(v, offsets, op, exclusive, reverse)
                want = np.zeros_like(v)
                for q in range(len(offsets) - 1):
                    ks = list(range(offsets[q], offsets[q + 1]))
                    for c in range(v.shape[1]):
                        acc = np.float32(S.IDENTITY[op])
                        for k in (ks[::-1] if reverse else ks):
                            x = v[k, c]
                            new = {"sum": lambda: np.float32(acc + x), "prod": lambda: np.float32(acc * x),
                                   "max": lambda: x if x > acc else acc, "min": lambda: x if x < acc else acc}[op]()
                            want[k, c] = acc if exclusive else new
                            acc = new
                np.testing.assert_array_equal(got, want)
        assert np.array_equal(S.scan(v[:, 0], offsets, op), S.scan(v[:, :1], offsets, op)[:, 0])


@pytest.mark.parametrize("op", S.OPS)
def test_float32_backward_recurrences_against_float64_autograd(op):
    """Every exclusive / reverse combination: |float32 sequence - float64 autograd| <= 2 n 2^-24 sum|terms| (the
    derivation: tests/scan_restate.py), n = 40 the fixture's longest ray; prod with exact zeros among values in [0.25, 1]."""
    offsets, v, g = fixture(op, 11)
    n = max(LENGTHS)
    for exclusive in (False, True):
        for reverse in (False, True):
            got = S.scan_backward(v, offsets, op, exclusive, reverse, g)
            want, terms = S.grad64(v, offsets, op, exclusive, reverse, g)
            assert got.dtype == np.float32 and np.all(np.isfinite(got))
            bound = 2 * n * 2.0 ** -24 * terms
            err = np.abs(got.astype(np.float64) - want)
            print(op, exclusive, reverse, "worst err / bound", (err[bound > 0] / bound[bound > 0]).max(), "entries", int((bound > 0).sum()))
            assert np.all(err <= bound + 1e-300)
            assert (want != 0).sum() > (30 if op in ("max", "min") else 150)
            if op in ("max", "min"):                   # mass is conserved over the positions that took a value
                out = S.scan(v, offsets, op, exclusive, reverse)
                np.testing.assert_allclose(want.sum(0), np.where(np.isfinite(out), g, 0).astype(np.float64).sum(0), rtol=0, atol=1e-9)
    if op == "prod":
        assert (v == 0).sum() >= 5


def test_restated_quantile():
    rng = np.random.default_rng(5)
    offsets, _, _ = fixture("sum", 5)
    T = int(offsets[-1])
    w = rng.uniform(0, 1, T).astype(np.float32)
    w[::4] = 0
    w[1::7] = -1.0
    w[2::13] = np.nan
    q = [0.0, 0.25, 0.5, 1.0]
    for normalize in (True, False):
        index, frac = S.quantile(w, offsets, q, normalize)
        assert index.shape == frac.shape == (len(offsets) - 1, 4) and frac.dtype == np.float32
        hit = index >= 0
        assert np.all(w[index[hit]] > 0) and np.all((frac >= 0) & (frac <= 1)) and np.all(frac[~hit] == 0)
        ray_of = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
        assert np.all(ray_of[index[hit]] == np.nonzero(hit)[0])
        assert np.all(np.diff(np.where(hit, index, T), axis=1) >= 0)                     # later targets cross no earlier
        if normalize:
            pos = np.array([np.any(w[offsets[r]:offsets[r + 1]] > 0) for r in range(len(offsets) - 1)])
            assert np.array_equal(hit.all(1), pos) and np.array_equal(hit.any(1), pos)
            # q = 0: the first positive sample, at its start; against float64 running sums
            c64 = np.cumsum(np.where(w > 0, w, 0).astype(np.float64))
            for r in np.nonzero(pos)[0]:
                first = offsets[r] + int(np.argmax(w[offsets[r]:offsets[r + 1]] > 0))
                assert index[r, 0] == first and frac[r, 0] == 0
                base = c64[offsets[r] - 1] if offsets[r] > 0 else 0.0
                total = c64[offsets[r + 1] - 1] - base
                k = index[r, 2]
                assert c64[k] - base >= 0.5 * total * (1 - 1e-5) and c64[k] - base - w[k] <= 0.5 * total * (1 + 1e-5)
        else:
            assert not hit[:, 3].all() and hit[:, 0].sum() > 5                          # a short ray's sum stays below 1
    assert S.quantile(w[:0], np.zeros(4, np.int64), q)[0].tolist() == [[-1] * 4] * 3


def test_restated_select_is_the_filtered_march():
    """select with keep = sigma > 0 on the unfiltered lists gives the lists of min_sigma = 0, array for array."""
    c = Case(depth=5, K=4, data_format="RGBA", width=48, height=48)
    ot, rays, opt = c.oracle_tree(), c.rays_np(), c.oracle_opts()
    every, pos = R.lists(ot, rays, opt), R.lists(ot, rays, opt, min_sigma=0.0)
    keep = ot.features[every.row, -1] > 0
    offsets, ray, row, depth, length, index = S.select(keep, every.offsets, every.ray, every.row, every.depth, every.length)
    for got, want in zip((offsets, row, ray, depth, length), pos):
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got, want)
    assert np.array_equal(index, np.nonzero(keep)[0]) and 1000 < index.shape[0] < keep.shape[0]
    # none and all
    none = S.select(np.zeros_like(keep), every.offsets, every.ray, every.row, every.depth, every.length)
    assert not none[0].any() and none[0].shape == every.offsets.shape and all(x.shape == (0,) for x in none[1:])
    full = S.select(np.ones_like(keep), every.offsets, every.ray, every.row, every.depth, every.length)
    np.testing.assert_array_equal(full[0], every.offsets)
    np.testing.assert_array_equal(full[5], np.arange(keep.shape[0]))
