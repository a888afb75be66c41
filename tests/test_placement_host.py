"""Where a tensor starts in its buffer, without a GPU: the C entry points whose kernels read tree.features as 16-byte
vectors refuse a table that is not 16-byte aligned before any launch (include/svoxt.h, "Alignment"), the sigma-only entry
points do not look at it, and the helper that realigns such a table at the Python boundary (csrc/_marshal.py, _aligned16).
The GPU half is tests/test_gpu_placement.py."""
import ctypes

import pytest
import torch

from svox_t_amd.csrc import _abi, _marshal

lib = _abi._lib
BASE = 0x10000                      # 64 KiB: aligned to anything asked for here; never dereferenced
F, D, C, OFF, SC, ORG, OUT, GOUT, GRAD, REC, AUX, WS, MASK, TAB = (BASE * i for i in range(1, 15))
PAYLOADS = {4: (_abi.FORMAT_RGBA, 0), 28: (_abi.FORMAT_SH, 9), 32: (_abi.FORMAT_RGBA, 0), 13: (_abi.FORMAT_SH, 4),
            8: (_abi.FORMAT_RGBA, 0), 16: (_abi.FORMAT_RGBA, 0)}


def _tree(K, features, M):
    t = _abi._CTree()
    t.features, t.M, t.K, t.N = features, M, K, 2
    t.data, t.child, t.n_internal, t.offset, t.scaling = D, C, 8, OFF, SC
    return t


def _rays(Q):
    r = _abi._CRays()
    r.origins = r.dirs = r.vdirs = ORG
    r.Q = Q
    return r


def _opts(K):
    fmt, bd = PAYLOADS[K]
    return _abi._COptions(1e-3, 1.0, fmt, bd, -1, -1, 0.0, 0, max(bd - 1, 0), 0.0, 0.0)


def _lists():
    return _abi._CLists(REC, AUX, 8, None, 0, None, 0, None, 0, None, 0, 0, None)       # dense lists of 8 samples


def _cols(K):
    fmt, bd = PAYLOADS[K]
    return K if fmt == _abi.FORMAT_RGBA else (K - 1) // bd + 1


def _planned_step(K, M, Q):
    """A svoxt_step planned for the same extents on an ALIGNED table (the plan holds no pointer to the table)."""
    step = _abi._CStep()
    t, r, o = _tree(K, F, M), _rays(Q), _opts(K)
    assert lib.svoxt_step_plan(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), 0, ctypes.byref(step)) == 0, lib.svoxt_last_error()
    return step


# name -> call(tree, rays, opts, K, M, Q): the entry points that reach a 16-byte read of tree.features
def _fwd(t, r, o, K, M, Q):
    return lib.svoxt_volume_render_fwd(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), OUT, None)


def _fwd_ws(t, r, o, K, M, Q):
    return lib.svoxt_volume_render_fwd_ws(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), OUT, None, 0, 0, None)


def _fwd_scratch(t, r, o, K, M, Q):
    return lib.svoxt_volume_render_fwd_scratch(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), OUT, ctypes.byref(_lists()), 0, None)


def _fwd_record(t, r, o, K, M, Q):
    return lib.svoxt_volume_render_fwd_record(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), OUT, ctypes.byref(_lists()), None)


def _bwd(t, r, o, K, M, Q):
    return lib.svoxt_volume_render_bwd(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), GOUT, _cols(K), GRAD, 0, None, 0, None)


def _bwd_replay(t, r, o, K, M, Q):
    return lib.svoxt_volume_render_bwd_replay(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), GOUT, _cols(K), GRAD, 0,
                                              ctypes.byref(_lists()), None, None)


def _step_plan(t, r, o, K, M, Q):
    return lib.svoxt_step_plan(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), 0, ctypes.byref(_abi._CStep()))


def _step_forward(t, r, o, K, M, Q):
    step = _planned_step(K, M, Q)
    return lib.svoxt_step_forward(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), OUT, ctypes.byref(step), WS, None)


def _step_backward(t, r, o, K, M, Q):
    step = _planned_step(K, M, Q)
    return lib.svoxt_step_backward(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), GOUT, GRAD, ctypes.byref(step), WS, None)


def _exp_table(t, r, o, K, M, Q):
    return lib.svoxt_exp_table_build(ctypes.byref(t), ctypes.c_float(0.0), MASK, TAB, None)


VECTOR_ENTRIES = {"svoxt_volume_render_fwd": _fwd, "svoxt_volume_render_fwd_ws": _fwd_ws, "svoxt_volume_render_fwd_scratch": _fwd_scratch,
                  "svoxt_volume_render_fwd_record": _fwd_record, "svoxt_volume_render_bwd": _bwd,
                  "svoxt_volume_render_bwd_replay": _bwd_replay, "svoxt_step_plan": _step_plan, "svoxt_step_forward": _step_forward,
                  "svoxt_step_backward": _step_backward, "svoxt_exp_table_build": _exp_table}
ALIGNMENT_WORDS = b"16-byte aligned"


@pytest.mark.parametrize("name", list(VECTOR_ENTRIES))
@pytest.mark.parametrize("K", [4, 28, 32])
@pytest.mark.parametrize("shift", [4, 8, 12])
def test_c_entry_refuses_a_misaligned_table_before_any_launch(name, K, shift):
    """SVOXT_ERR_INVALID from the argument checks, with a message that names the function, tree.features and the
    16-byte requirement: nothing reaches the HIP runtime (there is no GPU, and no pointer here can be dereferenced)."""
    call = VECTOR_ENTRIES[name]
    for M, Q in ((64, 16), (0, 0)):
        assert call(_tree(K, F + shift, M), _rays(Q), _opts(K), K, M, Q) == 1, (name, K, shift, M)
        msg = lib.svoxt_last_error()
        assert name.encode() in msg and b"tree.features" in msg and ALIGNMENT_WORDS in msg, msg


@pytest.mark.parametrize("name", list(VECTOR_ENTRIES))
@pytest.mark.parametrize("K,shift", [(13, 4), (13, 8), (13, 12), (4, 0), (28, 0), (32, 0)])
def test_c_entry_lets_the_other_tables_past_that_check(name, K, shift):
    """Rows that are no multiple of 4 floats are read float by float wherever they start, and an aligned table is an
    aligned table.  With no rays and no rows the calls end in the argument checks or just behind them, before any launch;
    whatever they answer, it is not the alignment refusal."""
    rc = VECTOR_ENTRIES[name](_tree(K, F + shift, 0), _rays(0), _opts(K), K, 0, 0)
    msg = lib.svoxt_last_error() if rc != 0 else b""
    assert not (b"tree.features" in msg and ALIGNMENT_WORDS in msg), (name, K, shift, rc, msg)
    if name != "svoxt_exp_table_build":                      # (which serves rows of 8 / 16 / 32 floats only)
        assert rc == 0, (name, K, shift, rc, msg)


@pytest.mark.parametrize("K", [8, 16, 32])
def test_exp_table_build_names_the_table_too(K):
    t = _tree(K, F, 64)
    assert lib.svoxt_exp_table_build(ctypes.byref(t), ctypes.c_float(0.0), MASK, TAB + 4, None) == 1
    assert b"svoxt_exp_table_build" in lib.svoxt_last_error() and ALIGNMENT_WORDS in lib.svoxt_last_error()
    t.exp_table = TAB + 8                                    # ... and a tree that carries a misaligned table of exponentials
    r, o = _rays(16), _opts(K)
    assert lib.svoxt_volume_render_fwd(ctypes.byref(t), ctypes.byref(r), ctypes.byref(o), OUT, None) == 1
    assert b"tree.exp_table" in lib.svoxt_last_error() and ALIGNMENT_WORDS in lib.svoxt_last_error()


def test_sigma_only_entries_do_not_ask_for_alignment():
    """Opacity, depth, counting, query, the sigma bitmask, the per-ray operators, ray_samples, the row-plan backward's count,
    ray_order, view_basis and the motion operators read single floats of the table: with no rays / points they return
    SVOXT_OK for a table 4 bytes off, K = 4 and 32 alike (nothing is launched: there is nothing to march)."""
    for K in (4, 32):
        t, r, o = _tree(K, F + 4, 0), _rays(0), _opts(K)
        a = (ctypes.byref(t), ctypes.byref(r), ctypes.byref(o))
        tm = _tree(K, F + 4, 0)
        tm.extra_data, tm.extra_rows, tm.extra_cols = TAB, 7, 3
        mo = _abi._CMotion(GOUT, 5, 8, GRAD, MASK, 2)
        calls = {
            "svoxt_opacity_render_fwd": lambda: lib.svoxt_opacity_render_fwd(*a, OUT, None),
            "svoxt_opacity_render_bwd": lambda: lib.svoxt_opacity_render_bwd(*a, GOUT, GRAD, None),
            "svoxt_render_depth": lambda: lib.svoxt_render_depth(*a, OUT, None),
            "svoxt_count_fwd": lambda: lib.svoxt_count_fwd(*a, OUT, None),
            "svoxt_query_fwd": lambda: lib.svoxt_query_fwd(ctypes.byref(t), ORG, 0, OUT, OUT, OUT, None, None),
            "svoxt_query_bwd": lambda: lib.svoxt_query_bwd(ctypes.byref(t), ORG, 0, GOUT, GRAD, None),
            "svoxt_sigma_mask_build": lambda: lib.svoxt_sigma_mask_build(ctypes.byref(t), ctypes.c_float(0.0), MASK, None),
            "svoxt_count_touched": lambda: lib.svoxt_count_touched(*a, OUT, GOUT, GRAD, None),
            "svoxt_ray_order": lambda: lib.svoxt_ray_order(*a, OUT, WS, 0, None),
            "svoxt_view_basis": lambda: lib.svoxt_view_basis(*a, OUT, None),
            "svoxt_depth_moments_fwd": lambda: lib.svoxt_depth_moments_fwd(*a, 0, OUT, None, 0, None),
            "svoxt_distortion_fwd": lambda: lib.svoxt_distortion_fwd(*a, OUT, None, 0, None),
            "svoxt_ray_samples_count": lambda: lib.svoxt_ray_samples_count(*a, None, OUT, None, 0, None),
            "svoxt_render_grad_rows_count": lambda: lib.svoxt_render_grad_rows_count(*a, OUT, None, 0, None),
            # the motion operators read sigma alone from the table (their joint-feature rows come from the aligned workspace)
            "svoxt_motion_render": lambda: lib.svoxt_motion_render(ctypes.byref(tm), ctypes.byref(r), ctypes.byref(o), OUT, OUT, OUT, OUT, None),
            "svoxt_motion_feature_render_fwd": lambda: lib.svoxt_motion_feature_render_fwd(
                ctypes.byref(t), ctypes.byref(mo), ctypes.byref(r), ctypes.byref(o), OUT, WS, 64, None),
        }
        for name, call in calls.items():
            assert call() == 0, (name, K, lib.svoxt_last_error())


# ------------------------------------------------------------------------------------------------- the realigning helper
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_aligned16_returns_an_aligned_tensor_as_it_is(dtype):
    t = torch.arange(96, dtype=dtype).view(12, 8)
    assert t.data_ptr() % 16 == 0
    assert _marshal._aligned16(t) is t
    four_on = torch.arange(100, dtype=dtype)[4:].view(12, 8)          # a view that starts on a 16-byte boundary again
    assert four_on.data_ptr() % 16 == 0 and _marshal._aligned16(four_on) is four_on


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_aligned16_copies_a_shifted_view(dtype, shift):
    buf = torch.arange(shift + 96 + 4, dtype=dtype)
    view = buf[shift:shift + 96].view(12, 8)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * shift
    before = buf.clone()
    got = _marshal._aligned16(view)
    assert got is not view and got.data_ptr() % 16 == 0 and got.data_ptr() != view.data_ptr()
    assert got.dtype == dtype and got.shape == view.shape and got.is_contiguous() and torch.equal(got, view)
    assert not got.requires_grad and torch.equal(buf, before)
    got.zero_()                                                       # its own storage: the caller's buffer is untouched
    assert torch.equal(buf, before)


def test_aligned16_of_a_tensor_that_requires_grad_is_a_plain_copy():
    buf = torch.randn(1 + 32)
    view = buf[1:].view(8, 4).requires_grad_()
    got = _marshal._aligned16(view)
    assert got.data_ptr() % 16 == 0 and not got.requires_grad and got.grad_fn is None and torch.equal(got, view.detach())
