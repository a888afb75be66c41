"""The deterministic render backward without a GPU: the C ABI's symbols and argument checks, and the anchors of the
restatement (tests/rowgrad_restate.py) -- its contributions are the C++ oracle's, its sum is the two-level chunk rule."""
import ctypes

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from svox_t_amd import synth
from svox_t_amd.csrc._abi import _COptions, _CRays, _CTree
from tests import rowgrad_restate as RG
from tests import rows_restate as R
from tests.util import Case

NAMES = ("svoxt_render_grad_rows_workspace_bytes", "svoxt_render_grad_rows_count", "svoxt_render_grad_rows_emit",
         "svoxt_render_grad_rows_plan", "svoxt_render_grad_rows_sweep", "svoxt_render_grad_rows_reduce")
BIG = 1 << 31


def test_symbols_and_abi_version():
    lib = ctypes.CDLL(_C.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _C.EXPORTS
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22
    assert ctypes.sizeof(_COptions) == 11 * 4                          # svoxt_options keeps its 11 fields
    assert callable(_C.volume_render_backward_rows)


def test_workspace_query():
    q = _C._lib.svoxt_render_grad_rows_workspace_bytes
    assert q(0, 0, 0, 4, 3, 0) == 0 and q(4096, 0, 3344, 28, 3, 9) == 0                  # no sample: no workspace
    for args in ((-1, 5, 4, 4, 3, 0), (BIG, 5, 4, 4, 3, 0), (4, -1, 4, 4, 3, 0), (4, BIG, 4, 4, 3, 0), (4, 5, -1, 4, 3, 0),
                 (4, 5, BIG, 4, 3, 0), (4, 5, 4, 0, 0, 0), (4, 5, 4, 4, -1, 0), (4, 5, 4, 4, 4, 0), (4, 5, 4, 4, 3, -1),
                 (4, 5, 4, 4, 3, 26), (4, BIG - 1, 4, 1 << 10, 1 << 9, 0), (4, 5, BIG - 1, 1 << 10, 3, 0)):
        assert q(*args) == -1, args
    for Q, T, M, K, C, bd in ((1, 1, 1, 4, 3, 0), (4096, 30000, 3344, 28, 3, 9), (640000, 6000000, 2000000, 28, 3, 9),
                              (4096, 30000, 3344, 4, 0, 0)):
        b = q(Q, T, M, K, C, bd)
        plan = _C._lib.svoxt_row_plan_workspace_bytes(T, M)
        assert b > 0 and b % 256 == 0
        # per sample 4 (C + 4) bytes and the plan's perm, per ray basis_dim + 1 floats, the plan's own arrays; every
        # piece padded to 256 bytes (14 pieces), the long rows' pieces by their bounds
        chunks = T // 256 + T // 257
        want = 4 * (C + 4) * T + 4 * T + 4 * (bd + 1) * Q + 4 * (M + 1) + 4 * (2 * (T // 257) + 1 + chunks) + 4 * chunks * K + plan
        assert want <= b <= want + 14 * 256, (b, want)


def specs(M=8, K=4, Q=16, fmt=0, bd=0, xform=False):
    """A tree / rays / options triple of plausible extents over fake (never dereferenced) pointers."""
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 63) & ~63
    t = _CTree()
    t.features, t.M, t.K, t.N, t.data, t.child, t.n_internal, t.offset, t.scaling = p, M, K, 2, p, p, 1, p, p
    if xform:
        t.xform, t.xform_dim = p, 3
    r = _CRays()
    r.origins, r.dirs, r.vdirs, r.Q = p, p, p, Q
    o = _COptions(1e-3, 1.0, fmt, bd, -1, -1, 0.0, 0, bd - 1, 0.0, 0.0)
    return t, r, o, ctypes.c_void_p(p), buf


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = _C._lib
    err = lib.svoxt_last_error
    count, emit, plan, sweep, reduce = (getattr(lib, n) for n in NAMES[1:])
    t, r, o, p, _keep = specs()
    odd4, odd1 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 1)
    B = 1 << 40
    by = ctypes.byref

    def all_three(tt, rr, oo, offsets=p, T=600, g=p, cols=4, ws=p, wsb=B):
        """(return code, message) of emit, sweep, plan and reduce for the arguments they share."""
        return [(emit(tt, rr, oo, offsets, T, g, cols, ws, wsb, None), err()),
                (sweep(tt, rr, oo, offsets, T, g, cols, ws, wsb, None), err()),
                (plan(tt, rr, oo, offsets, T, g, cols, p, ws, wsb, None), err()),
                (reduce(tt, rr, oo, offsets, T, g, cols, 0, 0, p, 0, ws, wsb, None), err())]

    def refused(results, text):
        for rc, msg in results:
            assert rc == 1 and text in msg, (rc, msg)

    # null specs
    refused(all_three(None, by(r), by(o)), b"tree is NULL")
    refused(all_three(by(t), None, by(o)), b"rays is NULL")
    refused(all_three(by(t), by(r), None), b"options is NULL")
    assert count(None, by(r), by(o), p, p, B, None) == 1 and b"tree is NULL" in err()
    assert count(by(t), by(r), by(o), None, p, B, None) == 1 and b"offsets is NULL" in err()
    # transformation_matrices are out of scope
    tx = specs(xform=True)[0]
    refused(all_three(by(tx), by(r), by(o)), b"transformation_matrices (tree.xform) are not served")
    assert count(by(tx), by(r), by(o), p, p, B, None) == 1 and b"transformation_matrices (tree.xform) are not served" in err()
    # negative extents
    rneg = specs(Q=-1)[1]
    refused(all_three(by(t), by(rneg), by(o)), b"negative ray count")
    for T in (-1, BIG):
        refused(all_three(by(t), by(r), by(o), T=T), b"T must be in [0, 2^31)")
    tneg = specs(M=-1)[0]
    refused(all_three(by(tneg), by(r), by(o)), b"bad feature table extents")
    # grad_out: its width is C + 1 (or 1), it is there
    for cols in (0, -1):
        refused(all_three(by(t), by(r), by(o), cols=cols), b"grad_cols must be >= 1")
    for cols in (2, 3, 5):
        refused(all_three(by(t), by(r), by(o), cols=cols), b"grad_out columns do not match get_out_data_dim")
    t28, _, o9, _, _ = specs(K=28, fmt=1, bd=9)
    for cols in (3, 28):
        refused(all_three(by(t28), by(r), by(o9), cols=cols), b"grad_out columns do not match get_out_data_dim")
    refused(all_three(by(t), by(r), by(o), g=None), b"offsets / grad_out is NULL")
    refused(all_three(by(t), by(r), by(o), offsets=None), b"offsets / grad_out is NULL")
    refused(all_three(by(t), by(r), by(o), offsets=odd4), b"is misaligned")
    refused(all_three(by(t), by(r), by(o), g=odd1), b"is misaligned")
    # the workspace
    need = lib.svoxt_render_grad_rows_workspace_bytes(16, 600, 8, 4, 3, 0)
    refused(all_three(by(t), by(r), by(o), ws=None), b"workspace is NULL")
    refused(all_three(by(t), by(r), by(o), wsb=need - 1), b"workspace smaller than svoxt_render_grad_rows_workspace_bytes")
    refused(all_three(by(t), by(r), by(o), ws=odd4), b"workspace is not 8-byte aligned")
    # the step's own arguments
    assert plan(by(t), by(r), by(o), p, 600, p, 4, None, p, B, None) == 1 and b"info is NULL or not 8-byte aligned" in err()
    assert plan(by(t), by(r), by(o), p, 600, p, 4, odd4, p, B, None) == 1 and b"info is NULL or not 8-byte aligned" in err()
    red = lambda n_long=0, n_chunks=0, grad=p, stride=0, T=600: reduce(by(t), by(r), by(o), p, T, p, 4, n_long, n_chunks, grad, stride,
                                                                       p, B, None)
    for stride in (1, 3):                                              # a row stride below K = 4
        assert red(stride=stride) == 1 and b"grad_stride smaller than data_dim" in err()
    for n_long, n_chunks in ((-1, 0), (9, 18), (3, 6)):
        assert red(n_long, n_chunks) == 1 and b"n_long must be in" in err()
    for n_long, n_chunks in ((2, 3), (2, 5), (0, 3)):
        assert red(n_long, n_chunks) == 1 and b"n_chunks must be in" in err()
    assert red(grad=None) == 1 and b"grad is NULL or not 4-byte aligned" in err()
    assert red(grad=odd1) == 1 and b"grad is NULL or not 4-byte aligned" in err()
    assert red(grad=None, T=0) == 1 and b"grad is NULL" in err()       # T = 0 still writes every element


def test_python_layer_refuses_what_is_out_of_scope():
    tree = svox.N3Tree(N=2, data_dim=4, init_reserve=4)
    r = svox.VolumeRenderer(tree)
    rays = svox.Rays(torch.zeros(2, 3), torch.ones(2, 3), torch.ones(2, 3))
    # (the tree is on the CPU: like every other entry, only the GPU path exists)
    with pytest.raises(RuntimeError, match="only the GPU"):
        r(tree.features, rays, deterministic=True)
    with pytest.raises(RuntimeError, match="only the GPU"):
        r.opacity_render(tree.features, rays, deterministic=True)
    spec = tree._spec(tree.features, transformation_matrices=torch.eye(3).repeat(tree.features.shape[0], 1, 1))
    with pytest.raises(RuntimeError, match="transformation_matrices are not served"):
        _C.volume_render_backward_rows(spec, None, r._get_options(), torch.zeros(2, 4))


# ------------------------------------------------------------------------------------------ anchors of the restatement
@pytest.mark.parametrize("fmt,K", [("SH9", 28), ("RGBA", 4)])
def test_contributions_are_the_oracles(fmt, K):
    """D = 5 shell tree (M = 3 344), 64 x 64 rays: the restatement's float32 contributions, summed per entry in float64,
    against the oracle's gradient -- float64 sums of the same float32 addends in two orders: n 2^-52 abs_sum apart at most."""
    c = Case(depth=5, K=K, data_format=fmt, width=64, height=64)
    ot, rays, opt = c.oracle_tree(), c.rays_np(), c.oracle_opts()
    assert ot.M == 3344
    g = synth.grad_output(c.Q, 4).numpy()
    want, absum, _tight = O.volume_render_backward(ot, *rays, opt, g, want_abs="both")
    con = RG.contributions(ot, rays, opt, g)
    assert con.row.shape[0] > 10000 and np.all(np.diff(con.ray) >= 0)
    got = np.zeros((ot.M, K))
    np.add.at(got, con.row, con.values.astype(np.float64))
    n = np.bincount(con.row, minlength=ot.M).astype(np.float64)[:, None]
    err = np.abs(got - want)
    bound = n * 2.0 ** -52 * absum
    assert np.all(err <= bound), (int((err > bound).sum()), float(err.max()))       # every entry
    assert np.count_nonzero(want) > 1000 and np.all(got[absum == 0] == 0)
    # and the chunked float32 sum of them is within the standard bound of that
    chunked = RG.grad(ot, rays, opt, g).astype(np.float64)
    assert np.all(np.abs(chunked - want) <= R.gamma(n) * absum + bound)


def test_the_sum_is_the_two_level_chunk_rule():
    """Every leaf of the D = 4 shell tree names row 0, thousands of samples on it, and the first ray that meets it has an
    upstream gradient of 1e9: the sequential float32 sum loses the later rays' contributions under that head, the chunk
    rule keeps them from the second chunk on.  The restatement gives the chunked value."""
    st = synth.shell_tree(4)
    data = np.where(st.data >= 0, np.where(st.data < st.n_features, 0, st.data), st.data).astype(np.int32)
    feats = np.array([[0.3, -0.2, 0.1, 0.7]], np.float32)
    ot = O.Tree(feats, data, st.child)
    o, d, v = (x.numpy() for x in synth.pinhole_rays(32, 32, c2w=synth.camera_pose()))
    opt = O.make_options()
    g = synth.grad_output(1024, 4).numpy()
    con = RG.contributions(ot, (o, d, v), opt, g)
    assert con.row.shape[0] > 1024 and not con.row.any()
    g[con.ray[0]] = 1e9
    con = RG.contributions(ot, (o, d, v), opt, g)
    vals = con.values
    partials = []
    for b in range(0, vals.shape[0], 256):
        acc = np.zeros(4, np.float32)
        for x in vals[b:b + 256]:
            acc = np.float32(acc + x)
        partials.append(acc)
    chunked = partials[0]
    for x in partials[1:]:
        chunked = np.float32(chunked + x)
    got = RG.grad(ot, (o, d, v), opt, g)
    assert got.shape == (1, 4)
    np.testing.assert_array_equal(got[0], chunked)
    assert np.any(got[0] != R.sum_sequential(vals))
