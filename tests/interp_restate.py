"""A plain numpy restatement of N3Tree.interp (include/svoxt.h, "interp"): the stencil with its own float32 descent and
its own integer corner descents, the value, the table gradient (through tests/rows_restate.py's chunked order) and the
point gradient, float32 operation by operation.  Slow and obvious on purpose; tests compare the GPU's bits against it.

Every float array here is float32 and every operation on two of them is ONE float32 operation (numpy rounds each)."""
from collections import namedtuple

import numpy as np

from tests import rows_restate as R

F = np.float32
CLAMP_HI = F(1.0 - 1e-6)
DEEPER = 64
Tree = namedtuple("Tree", "child data N M offset scaling")     # child / data flat int32 over the nodes in use
Located = namedtuple("Located", "slot own depth cube_sz l cell side cell_ok clamped")
Stencil = namedtuple("Stencil", "rows weights s f g cube_sz clamped")


def tree_of(child, data, M, offset=(0, 0, 0), scaling=(1, 1, 1)):
    child = np.asarray(child, np.int32)
    return Tree(child.reshape(-1).astype(np.int64), np.asarray(data, np.int32).reshape(-1).astype(np.int64), int(child.shape[1]), int(M),
                np.asarray(offset, F), np.asarray(scaling, F))


def _row(tree, slot):
    w = tree.data[slot]
    return np.where((w >= 0) & (w < tree.M), w, -1)


def locate(tree, points):
    """Step 1 for points float32 [Q, 3]: the transform, the clamp, the reference's float descent with its digits kept."""
    N = tree.N
    p = np.asarray(points, F)
    t = (tree.offset[None, :] + (tree.scaling[None, :] * p).astype(F)).astype(F)
    c = np.maximum(F(0), np.minimum(CLAMP_HI, t)).astype(F)
    Q = p.shape[0]
    loc = c.copy()
    node = np.zeros(Q, np.int64)
    slot = np.zeros(Q, np.int64)
    levels = np.zeros(Q, np.int64)
    cube = np.full(Q, F(N), F)
    cell = np.zeros((Q, 3), np.int64)
    side = np.ones(Q, np.int64)
    ok = np.ones(Q, bool)
    live = np.ones(Q, bool)
    while live.any():
        a = np.nonzero(live)[0]
        x = (loc[a] * F(N)).astype(F)
        fl = np.floor(x).astype(F)
        loc[a] = (x - fl).astype(F)
        dg = np.clip(fl.astype(np.int64), 0, N - 1)
        s = ((node[a] * N + dg[:, 0]) * N + dg[:, 1]) * N + dg[:, 2]
        levels[a] += 1
        grow = ok[a] & (side[a] * N < 2 ** 31)
        cell[a] = np.where(grow[:, None], cell[a] * N + dg, cell[a])
        side[a] = np.where(grow, side[a] * N, side[a])
        ok[a] = grow
        slot[a] = s
        ch = tree.child[s]
        leaf = ch == 0
        live[a[leaf]] = False
        b = a[~leaf]
        cube[b] = (cube[b] * F(N)).astype(F)
        node[b] += ch[~leaf]
    return Located(slot, _row(tree, slot), levels - 1, cube, loc, cell, side, ok, c != t)


def cell_row(tree, t, d, side):
    """Step 4 for ONE cell t (3 ints) of level d inside the cube: the row, or -1."""
    N, n3 = tree.N, tree.N ** 3
    n = tree.child.shape[0] // n3
    node, pw = 0, side // N
    for _ in range(d + 1):
        s = node * n3 + (((t[0] // pw) % N) * N + (t[1] // pw) % N) * N + (t[2] // pw) % N
        ch = int(tree.child[s])
        if ch == 0:
            return int(_row(tree, s))
        node += ch
        if node <= 0 or node >= n:
            return -1
        pw //= N
    dg = N // 2
    for _ in range(DEEPER):
        s = node * n3 + (dg * N + dg) * N + dg
        ch = int(tree.child[s])
        if ch == 0:
            return int(_row(tree, s))
        node += ch
        if node <= 0 or node >= n:
            return -1
        if N % 2 == 0:
            dg = 0
    return -1


def stencil(tree, points, fill="self"):
    """Steps 1 - 6: rows int32 [Q, 8], weights float32 [Q, 8] (and s, f, g, cube_sz, clamped for the point gradient)."""
    L = locate(tree, points)
    Q = L.slot.shape[0]
    u = (L.l - F(0.5)).astype(F)
    s = np.where(u < 0, -1, 1).astype(np.int64)
    f = np.abs(u).astype(F)
    g = (F(1.0) - f).astype(F)
    rows = np.full((Q, 8), -1, np.int32)
    weights = np.zeros((Q, 8), F)
    for j in range(8):
        b = np.array([(j >> 2) & 1, (j >> 1) & 1, j & 1])
        m = np.where(b[None, :] == 1, f, g).astype(F)
        weights[:, j] = ((m[:, 0] * m[:, 1]).astype(F) * m[:, 2]).astype(F)
        for q in range(Q):
            own = int(L.own[q])
            if own < 0:
                continue
            if j == 0:
                rows[q, j] = own
                continue
            row = own if fill == "self" else -1
            if L.cell_ok[q]:
                t = L.cell[q] + b * s[q]
                if (t >= 0).all() and (t < L.side[q]).all():
                    r = cell_row(tree, [int(v) for v in t], int(L.depth[q]), int(L.side[q]))
                    if r >= 0:
                        row = r
            rows[q, j] = row
    return Stencil(rows, weights, s, f, g, L.cube_sz, L.clamped)


def _cols(cols, K):
    return np.arange(K) if cols is None else np.asarray(cols, np.int64)


def value(table, rows, weights, cols=None):
    """out[q, jc] = acc over ascending j of acc + w_j * table[rows[q, j], cols[jc]], corners outside [0, M) skipped."""
    table = np.asarray(table, F)
    M, K = table.shape
    cs = _cols(cols, K)
    out = np.zeros((rows.shape[0], cs.shape[0]), F)
    for j in range(8):
        r = rows[:, j].astype(np.int64)
        k = (r >= 0) & (r < M)
        v = table[r[k]][:, cs]
        out[k] = (out[k] + (weights[k, j][:, None] * v).astype(F)).astype(F)
    return out


def table_grad(g, rows, weights, M, K, cols=None):
    """G [M, K]: reduce_rows' chunked sum of weights[e] * g[e >> 3] over the entries of every row, 0 elsewhere."""
    g = np.asarray(g, F)
    vals = (weights.reshape(-1)[:, None] * np.repeat(g, 8, axis=0)).astype(F)
    return R.gather_grad(vals, rows.reshape(-1), M, K, None if cols is None else np.asarray(cols))


def point_grad(tree, st, table, g, cols=None):
    """grad_points [Q, 3] for the stencil st of a tree (its scaling) and the upstream gradient g [Q, C]."""
    table = np.asarray(table, F)
    g = np.asarray(g, F)
    M, K = table.shape
    cs = _cols(cols, K)
    Q = st.rows.shape[0]
    D = np.zeros((Q, 8), F)
    for j in range(8):
        r = st.rows[:, j].astype(np.int64)
        k = (r >= 0) & (r < M)
        acc = np.zeros(int(k.sum()), F)
        v = table[r[k]][:, cs]
        for jc in range(cs.shape[0]):
            acc = (acc + (g[k, jc] * v[:, jc]).astype(F)).astype(F)
        D[k, j] = acc
    out = np.zeros((Q, 3), F)
    for a in range(3):
        a1, a2 = [x for x in range(3) if x != a]
        S = np.zeros(Q, F)
        for j in range(8):
            b = [(j >> 2) & 1, (j >> 1) & 1, j & 1]
            m1 = st.f[:, a1] if b[a1] else st.g[:, a1]
            m2 = st.f[:, a2] if b[a2] else st.g[:, a2]
            m = (m1 * m2).astype(F)
            sm = m if b[a] else (-m).astype(F)
            S = (S + (sm * D[:, j]).astype(F)).astype(F)
        v = (((S * st.s[:, a].astype(F)).astype(F) * st.cube_sz).astype(F) * tree.scaling[a]).astype(F)
        out[:, a] = np.where(st.clamped[:, a], F(0), v)
    return out


# ----------------------------------------------------------------------------------------------------------- float64
def value64(table, rows, l, cols=None):
    """The float64 sum with EXACT weights (from the float32 leaf-local coordinates l, which the descent forms without a
    choice), and sum_j w_j |v_j| for the bound."""
    table = np.asarray(table, np.float64)
    M, K = table.shape
    cs = _cols(cols, K)
    u = np.asarray(l, np.float64) - 0.5
    f, g = np.abs(u), 1.0 - np.abs(u)
    out = np.zeros((rows.shape[0], cs.shape[0]))
    mag = np.zeros_like(out)
    wsum = np.zeros(rows.shape[0])
    for j in range(8):
        b = [(j >> 2) & 1, (j >> 1) & 1, j & 1]
        w = np.prod([f[:, a] if b[a] else g[:, a] for a in range(3)], axis=0)
        wsum += w
        r = rows[:, j].astype(np.int64)
        k = (r >= 0) & (r < M)
        v = table[r[k]][:, cs]
        out[k] += w[k, None] * v
        mag[k] += w[k, None] * np.abs(v)
    return out, mag, wsum


def uniform_tree(levels, N=2):
    """(child [n, N, N, N], data [n, N, N, N, 1], parent_depth [n, 2], L): the full tree with `levels` levels of nodes,
    nodes in breadth-first order; leaf l in slot order names row l."""
    n3 = N ** 3
    counts = [n3 ** k for k in range(levels)]
    n = sum(counts)
    child = np.zeros((n, N, N, N), np.int32)
    pd = np.zeros((n, 2), np.int32)
    flat = child.reshape(n, n3)
    start = 0
    for k in range(levels - 1):
        nxt = start + counts[k]
        for i in range(counts[k]):
            for s in range(n3):
                kid = nxt + i * n3 + s
                flat[start + i, s] = kid - (start + i)
                pd[kid] = ((start + i) * n3 + s, k + 1)
        start = nxt
    leaf = flat.reshape(-1) == 0
    L = int(leaf.sum())
    data = np.full(n * n3, -1, np.int32)
    data[leaf] = np.arange(L, dtype=np.int32)
    return child, data.reshape(n, N, N, N, 1), pd, L


def leaf_centres(tree):
    """float64 [slots, 3] centre and int depth of every slot (meaningful at leaf slots), by a walk from the root."""
    N, n3 = tree.N, tree.N ** 3
    n = tree.child.shape[0] // n3
    lo = np.zeros((n * n3, 3))
    depth = np.zeros(n * n3, np.int64)
    stack = [(0, np.zeros(3), 0)]
    while stack:
        node, base, d = stack.pop()
        size = float(N) ** -(d + 1)
        for s in range(n3):
            idx = node * n3 + s
            dg = np.array([s // (N * N), (s // N) % N, s % N], np.float64)
            lo[idx] = base + dg * size
            depth[idx] = d
            if tree.child[idx] != 0:
                stack.append((node + int(tree.child[idx]), lo[idx].copy(), d + 1))
    return lo + 0.5 * (float(N) ** -(depth[:, None] + 1.0)), depth
