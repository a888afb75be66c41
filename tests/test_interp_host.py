"""N3Tree.interp without a GPU: the numpy restatement (tests/interp_restate.py) against float64, affine reproduction on a
full uniform tree, the argument checks of the new exports (which come before any HIP call) and the Python refusals.

Bounds (u = 2^-24, one float32 rounding):
  value     12 u sum_j w_j |v_j|: every weight carries 3 roundings, the sum 8 products and adds (11 to first order per
            term, 12 with room for the second); held to HALF here, as DESIGN.md section 5 holds its references.
            Measured on this lattice: 0.37 of the bound.
  weights   w >= 0, |sum w - 1| <= 2^-19.
  point gradient   (16 + C) u sum_j (m_a' m_a'') sum_c |g_c v_jc| cube_sz |scaling_a|: the analogous count -- D_j is C
            products and adds (+1 for the product with it), the two factors m one rounding each (g = 1 - f) and their
            product one, eight adds, three trailing products -- held to half as well.
The float64 references take their weights from the float32 leaf-local coordinates l: the descent forms l without a
choice (exactly for N = 2), and a reference that re-derived l in float64 from world coordinates would differ from the
definition by cube_sz roundings of the transform, which is not the error under test."""
import ctypes
import os

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from svox_t_amd import synth
from tests import interp_restate as IR

G = os.path.join(os.path.dirname(__file__), "golden")
U = 2.0 ** -24
NEW = ("svoxt_interp_stencil", "svoxt_interp_rows_fwd", "svoxt_interp_rows_bwd_workspace_bytes", "svoxt_interp_rows_bwd",
       "svoxt_interp_points_bwd")
_X = _C._extras


def lattice(levels=4, K=5, seed=0):
    """A uniform 16^3 lattice (N = 2, four levels of nodes): (restatement tree, table, points with exact centres and faces)."""
    child, data, _, L = IR.uniform_tree(levels)
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((L, K)).astype(np.float32)
    t = IR.tree_of(child, data, L)
    side = 2 ** levels
    p = rng.random((4000, 3)).astype(np.float32)
    cells = rng.integers(0, side, (600, 3))
    centres = ((cells + 0.5) / side).astype(np.float32)
    faces = centres.copy()
    faces[np.arange(600), rng.integers(0, 3, 600)] = (cells[:, 0] / side).astype(np.float32)
    outside = (rng.random((200, 3)) * 3 - 1).astype(np.float32)
    edge = np.array([[0, 0, 0], [1, 1, 1], [0, 1, 0.5], [1, 0.25, 0]], np.float32)
    return t, table, np.concatenate([p, centres, faces, outside, edge])


_CACHE = {}


def lattice_stencil():
    if "lat" not in _CACHE:
        t, table, pts = lattice()
        _CACHE["lat"] = (t, table, pts, IR.stencil(t, pts), IR.locate(t, pts))
    return _CACHE["lat"]


def test_restatement_value_and_weights_against_float64():
    t, table, pts, st, L = lattice_stencil()
    got = IR.value(table, st.rows, st.weights)
    want, mag, wsum = IR.value64(table, st.rows, L.l)
    bound = 12 * U * mag
    ratio = (np.abs(got.astype(np.float64) - want) / np.maximum(bound, 1e-300)).max()
    print("value: worst error / bound =", ratio)
    assert ratio <= 0.5
    assert (st.weights >= 0).all()
    dev = np.abs(st.weights.astype(np.float64).sum(axis=1) - 1.0).max()
    print("weights: worst |sum w - 1| / 2^-24 =", dev / U)
    assert dev <= 2.0 ** -19
    assert np.abs(wsum - 1.0).max() <= 1e-12
    # exact leaf centres reproduce the own row bit for bit
    centres = slice(4000, 4600)
    own = st.rows[centres, 0]
    np.testing.assert_array_equal(got[centres].view(np.uint32), table[own].view(np.uint32))
    assert (st.weights[centres, 0] == 1).all() and (st.weights[centres, 1:] == 0).all()


def test_restatement_point_gradient_against_float64_autograd():
    t, table, pts, st, L = lattice_stencil()
    rng = np.random.default_rng(1)
    scaling = np.array([0.5, 2.0, 1.25], np.float32)
    tw = IR.Tree(t.child, t.data, t.N, t.M, t.offset, scaling)             # the chain factor alone: the stencil is st's
    for cols in (None, [4, 1]):
        C = table.shape[1] if cols is None else len(cols)
        g = rng.standard_normal((pts.shape[0], C)).astype(np.float32)
        got = IR.point_grad(tw, st, table, g, cols)
        l = torch.tensor(L.l.astype(np.float64), requires_grad=True)
        u = l - 0.5
        f, gg = u.abs(), 1.0 - u.abs()
        v = torch.tensor(table.astype(np.float64))[:, list(range(table.shape[1])) if cols is None else cols]
        out = 0
        mag = np.zeros((pts.shape[0], 3))
        for j in range(8):
            b = [(j >> 2) & 1, (j >> 1) & 1, j & 1]
            m = [f[:, a] if b[a] else gg[:, a] for a in range(3)]
            vj = v[torch.tensor(st.rows[:, j].astype(np.int64))]
            out = out + (m[0] * m[1] * m[2])[:, None] * vj
            gv = (np.abs(g.astype(np.float64)) * np.abs(vj.numpy())).sum(axis=1)
            md = [x.detach().numpy() for x in m]
            for a in range(3):
                a1, a2 = [x for x in range(3) if x != a]
                mag[:, a] += md[a1] * md[a2] * gv
        out.backward(torch.tensor(g.astype(np.float64)))
        chain = L.cube_sz.astype(np.float64)[:, None] * scaling.astype(np.float64)[None, :]
        want = np.where(L.clamped, 0.0, l.grad.numpy() * chain)
        bound = (16 + C) * U * mag * np.abs(chain)
        ok = ~L.clamped & (np.abs(L.l - 0.5) > 0)                          # |u| has no derivative at the centre plane: s = +1 there by definition
        ratio = (np.abs(got.astype(np.float64) - want)[ok] / np.maximum(bound[ok], 1e-300)).max()
        print("point gradient: worst error / bound =", ratio, "cols", cols)
        assert ratio <= 0.5
        assert (got[L.clamped] == 0).all() and L.clamped.any()


def test_affine_reproduction_on_a_full_uniform_tree():
    """Rows that are an affine function of the leaf centre with dyadic coefficients: half a cell inside the cube and
    further, interp gives that function of the point."""
    child, data, _, Lc = IR.uniform_tree(3)
    t = IR.tree_of(child, data, Lc)
    centre, _ = IR.leaf_centres(t)
    a0 = np.array([0.5, -2.0, 0.25])
    A = np.array([[1.0, -0.5, 2.0], [0.25, 0.0, -4.0], [-1.0, 1.0, 0.125]])     # [column, axis]
    leaf = t.child == 0
    table = np.zeros((Lc, 3), np.float32)
    table[t.data[leaf]] = (a0[None, :] + centre[leaf] @ A.T).astype(np.float32)
    assert np.array_equal(table.astype(np.float64)[t.data[leaf]], a0[None, :] + centre[leaf] @ A.T)   # dyadic: exact
    rng = np.random.default_rng(2)
    h = 0.5 / 8
    pts = (h + rng.random((3000, 3)) * (1 - 2 * h)).astype(np.float32)
    pts = np.clip(pts, np.float32(h), np.float32(1 - h))
    st = IR.stencil(t, pts, "zero")
    assert (st.rows >= 0).all()                                            # every corner inside the cube, both fills alike
    np.testing.assert_array_equal(st.rows, IR.stencil(t, pts, "self").rows)
    got = IR.value(table, st.rows, st.weights).astype(np.float64)
    want = a0[None, :] + pts.astype(np.float64) @ A.T
    mag = (st.weights.astype(np.float64)[:, :, None] * np.abs(table.astype(np.float64)[st.rows])).sum(axis=1)
    ratio = (np.abs(got - want) / (12 * U * mag)).max()
    print("affine: worst error / bound =", ratio)
    assert ratio <= 1.0


def test_corner_rows_are_the_query_at_the_cell_centres():
    """The restatement's corner descent against its own point descent at the float64 cell centres (N = 2: exact), on a
    tree with level changes; the GPU file repeats this against tree.forward."""
    g = np.load(os.path.join(G, "topology_points_a.npz"))
    child = g["child"]
    leaf = child.reshape(-1) == 0
    Lc = int(leaf.sum())
    data = np.full(child.size, synth.EMPTY_SENTINEL, np.int32)
    words = np.arange(Lc, dtype=np.int32)
    words[2::3] = synth.EMPTY_SENTINEL
    data[leaf] = words
    t = IR.tree_of(child, data, Lc)
    rng = np.random.default_rng(3)
    pts = rng.random((1500, 3)).astype(np.float32)
    L = IR.locate(t, pts)
    for fill in ("self", "zero"):
        st = IR.stencil(t, pts, fill)
        size = 1.0 / L.side.astype(np.float64)
        seen = 0
        for j in range(8):
            b = np.array([(j >> 2) & 1, (j >> 1) & 1, j & 1])
            cellj = L.cell + b[None, :] * st.s
            X = (cellj + 0.5) * size[:, None]
            inside = ((X > 0) & (X < 1)).all(axis=1)
            q = IR.locate(t, X.astype(np.float32)).own
            has = inside & (q >= 0)
            want = np.where(has, q, L.own if fill == "self" else -1)
            want = np.where(L.own < 0, -1, want)
            np.testing.assert_array_equal(st.rows[:, j], want)
            seen += int((has & (L.own >= 0) & (q != L.own)).sum())
        assert seen > 1000
    assert len(set(L.depth.tolist())) > 1                                  # the tree has level changes


def test_new_symbols_and_abi_version():
    lib = ctypes.CDLL(_C.LIB_PATH)
    header = open(os.path.join(os.path.dirname(G), "..", "include", "svoxt.h")).read()
    for nm in NEW:
        assert nm in _C.EXPORTS and hasattr(lib, nm) and nm + "(" in header, nm
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22
    for nm in ("interp_stencil", "interp_rows_fwd", "interp_rows_bwd", "interp_points_bwd"):
        assert callable(getattr(_X, nm))
    assert _X.INTERP_FILLS == {"self": 0, "zero": 1}


def _fake_tree(buf, M=10, K=4, N=2, n=4):
    t = _C._CTree()
    p = ctypes.addressof(buf)
    t.features, t.data, t.child, t.offset, t.scaling = p, p, p, p, p
    t.M, t.K, t.N, t.n_internal = M, K, N, n
    return t


def test_c_abi_argument_checks_come_before_any_hip_call():
    lib = _C._lib
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    err = lambda: lib.svoxt_last_error()                                       # noqa: E731
    t = _fake_tree(buf)
    big = 1 << 30
    stn = lambda **k: lib.svoxt_interp_stencil(k.get("tree", ctypes.byref(t)), k.get("points", p), k.get("Q", 8), k.get("fill", 0),   # noqa: E731
                                               k.get("rows", p), k.get("weights", p), None)
    assert stn(tree=None) == 1 and b"tree is NULL" in err()
    assert stn(tree=ctypes.byref(_fake_tree(buf, N=17))) == 1 and b"branching" in err()
    assert stn(tree=ctypes.byref(_fake_tree(buf, N=1))) == 1
    assert stn(Q=-1) == 1 and b"Q must be" in err()
    assert stn(Q=1 << 28) == 1 and b"8 Q < 2^31" in err()
    assert stn(fill=2) == 1 and b"fill must be" in err()
    assert stn(fill=-1) == 1
    assert stn(points=None) == 1 and b"NULL" in err()
    assert stn(rows=None) == 1 and stn(weights=None) == 1
    assert stn(points=odd) == 1 and b"misaligned" in err()
    assert stn(Q=0, points=None, rows=None, weights=None) == 0
    fwd = lambda **k: lib.svoxt_interp_rows_fwd(k.get("table", p), k.get("M", 10), k.get("K", 4), k.get("rows", p), k.get("weights", p),   # noqa: E731
                                                k.get("Q", 8), k.get("cols", None), k.get("n_cols", 0), k.get("out", p), None)
    assert fwd(Q=-1) == 1 and fwd(Q=1 << 28) == 1 and b"Q must be" in err()
    assert fwd(M=-1) == 1 and b"M must be" in err()
    assert fwd(K=0) == 1 and b"K must be" in err()
    assert fwd(cols=p, n_cols=0) == 1 and b"cols / n_cols" in err()
    assert fwd(n_cols=2) == 1 and fwd(cols=p, n_cols=5) == 1
    assert fwd(M=1 << 30, K=1 << 10) == 1 and b"2^38" in err()
    assert fwd(rows=None) == 1 and b"NULL" in err()
    assert fwd(weights=None) == 1 and fwd(out=None) == 1
    assert fwd(table=None) == 1 and b"table is NULL" in err()
    assert fwd(out=odd) == 1 and b"misaligned" in err()
    assert fwd(Q=0, rows=None, weights=None, out=None, table=None) == 0
    ws = lib.svoxt_interp_rows_bwd_workspace_bytes
    assert ws(-1, 4) == -1 and ws(1 << 31, 4) == -1 and ws(5, 0) == -1 and ws(1 << 30, 1 << 10) == -1
    assert ws(0, 4) == 0 and ws(3, 4) >= 48 and ws(3, 4) % 256 == 0
    bwd = lambda **k: lib.svoxt_interp_rows_bwd(k.get("g", p), k.get("weights", p), k.get("Q", 100), k.get("C", 4), k.get("row_ptr", p),   # noqa: E731
                                                k.get("perm", p), k.get("M", 10), k.get("long_rows", p), k.get("lcp", p), k.get("cl", p),
                                                k.get("n_long", 0), k.get("n_chunks", 0), k.get("cols", None), k.get("n_cols", 0),
                                                k.get("K", 4), k.get("grad", p), k.get("ws", p), k.get("bytes", big), None)
    assert bwd(Q=-1) == 1 and bwd(Q=1 << 28) == 1 and b"8 Q < 2^31" in err()
    assert bwd(C=3) == 1 and b"one column per selected column" in err()
    assert bwd(cols=p, n_cols=2, C=4) == 1
    assert bwd(n_long=-1) == 1 and b"n_long" in err()
    assert bwd(n_long=4) == 1                                               # 800 entries hold at most 3 long rows
    assert bwd(n_long=1, n_chunks=1) == 1 and b"n_chunks" in err()
    assert bwd(n_long=1, n_chunks=5) == 1
    assert bwd(grad=None) == 1 and b"grad / row_ptr is NULL" in err()
    assert bwd(g=None) == 1 and b"grad_out / weights / perm is NULL" in err()
    assert bwd(n_long=1, n_chunks=2, long_rows=None) == 1 and b"long_rows" in err()
    assert bwd(grad=odd) == 1 and b"misaligned" in err()
    assert bwd(n_long=1, n_chunks=2, ws=None) == 1 and b"workspace is NULL" in err()
    assert bwd(n_long=1, n_chunks=2, bytes=16) == 1 and b"workspace smaller" in err()
    assert bwd(M=0, grad=None, row_ptr=None) == 0
    pb = lambda **k: lib.svoxt_interp_points_bwd(k.get("tree", ctypes.byref(t)), k.get("points", p), k.get("Q", 8), k.get("rows", p),   # noqa: E731
                                                 k.get("table", p), k.get("M", 10), k.get("K", 4), k.get("cols", None), k.get("n_cols", 0),
                                                 k.get("g", p), k.get("out", p), None)
    assert pb(tree=None) == 1 and b"tree is NULL" in err()
    assert pb(tree=ctypes.byref(_fake_tree(buf, N=17))) == 1
    assert pb(Q=-1) == 1 and pb(Q=1 << 28) == 1
    assert pb(K=0) == 1 and pb(n_cols=1) == 1 and b"cols / n_cols" in err()
    assert pb(points=None) == 1 and b"NULL" in err()
    assert pb(rows=None) == 1 and pb(g=None) == 1 and pb(out=None) == 1
    assert pb(table=None) == 1 and b"table is NULL" in err()
    assert pb(g=odd) == 1 and b"misaligned" in err()
    assert pb(Q=0, points=None, rows=None, g=None, out=None) == 0


def test_python_refusals():
    tree = svox.N3Tree(N=2, data_dim=4, init_refine=1)                         # a CPU tree
    pts = torch.rand(5, 3)
    for call in (lambda: tree.interp(pts), lambda: tree.interp_stencil(pts), lambda: tree.interp(svox.LocalIndex(pts)),
                 lambda: tree.interp(pts.clone().requires_grad_(True))):
        with pytest.raises(RuntimeError, match="GPU") as e:
            call()
        assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(RuntimeError, match="fill must be"):
        tree.interp(pts, fill="mirror")
    with pytest.raises(RuntimeError, match="fill must be"):
        tree.interp_stencil(pts, fill="edge")
    rows = torch.zeros(5, 8, dtype=torch.int32)
    w = torch.zeros(5, 8)
    st = svox.InterpStencil(rows, w)
    assert len(st) == 5 and tuple(st)[0] is rows and tuple(st)[1] is w
    with pytest.raises(RuntimeError, match=r"rows must be int32 \[Q, 8\]"):
        svox.InterpStencil(rows[:, :7], w)
    with pytest.raises(RuntimeError, match="weights must be float32"):
        svox.InterpStencil(rows, w.double())
    with pytest.raises(RuntimeError, match="GPU"):
        svox.interp_rows(st, tree.features)
    with pytest.raises(RuntimeError, match="GPU"):
        st.row_plan(10)
    with pytest.raises(RuntimeError, match="stencil must be an InterpStencil"):
        svox.interp_rows((rows, w), tree.features)
    with pytest.raises(RuntimeError, match="table must be float32"):
        svox.interp_rows(st, tree.features.double())
    # the operator layer: values, shapes and dtypes before devices
    spec = tree._spec(tree.features.detach())
    with pytest.raises(RuntimeError, match="fill must be"):
        _X.interp_stencil(spec, pts, "mirror")
    with pytest.raises(RuntimeError, match=r"indices must be float32 \[Q, 3\]"):
        _X.interp_stencil(spec, pts[:, :2])
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _X.interp_stencil(spec, pts)
    table = tree.features.detach()
    with pytest.raises(RuntimeError, match=r"rows must be int32 \[Q, 8\]"):
        _X.interp_rows_fwd(table, rows.long(), w)
    with pytest.raises(RuntimeError, match="weights must be float32"):
        _X.interp_rows_fwd(table, rows, w[:4])
    with pytest.raises(RuntimeError, match="table must be float32"):
        _X.interp_rows_fwd(table.double(), rows, w)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _X.interp_rows_fwd(table, rows, w)
    with pytest.raises(RuntimeError, match="plan must be a row plan"):
        _X.interp_rows_bwd(torch.zeros(5, 4), w, None)
    with pytest.raises(RuntimeError, match=r"rows must be int32 \[Q, 8\]"):
        _X.interp_points_bwd(spec, pts, rows[:4], table, torch.zeros(5, 4))
    with pytest.raises(RuntimeError, match=r"grad_out must be float32 \[Q, C\]"):
        _X.interp_points_bwd(spec, pts, rows, table, torch.zeros(5, 3))


def test_ray_samples_points_refusals_and_values():
    off = torch.tensor([0, 2, 2, 3])
    s = svox.RaySamples(off, torch.tensor([0, 0, 2], dtype=torch.int32), torch.zeros(3, dtype=torch.int32),
                        torch.tensor([1.0, 2.0, 0.5]), torch.tensor([0.5, 0.25, 2.0]))
    o = torch.tensor([[0.0, 0, 0], [9, 9, 9], [1, 1, 1]])
    d = torch.tensor([[1.0, 0, 0], [0, 1, 0], [0, 0, 2]])
    rays = svox.Rays(o, d, d)
    np.testing.assert_array_equal(s.points(rays).numpy(), [[1.25, 0, 0], [2.125, 0, 0], [1, 1, 4]])
    np.testing.assert_array_equal(s.points(rays, at="entry").numpy(), [[1, 0, 0], [2, 0, 0], [1, 1, 2]])
    assert not s.points(svox.Rays(o.clone().requires_grad_(True), d, d)).requires_grad
    with pytest.raises(RuntimeError, match="at must be"):
        s.points(rays, at="exit")
    with pytest.raises(RuntimeError, match="camera-mode and NDC"):
        s.points(torch.eye(4))
    with pytest.raises(RuntimeError, match="camera-mode and NDC"):
        s.points(dict(c2w=torch.eye(4), width=8, height=8))
    with pytest.raises(RuntimeError, match="rays the samples were marched from"):
        s.points(svox.Rays(o[:2], d[:2], d[:2]))
    with pytest.raises(RuntimeError, match="rays the samples were marched from"):
        s.points(svox.Rays(o.double(), d, d))
