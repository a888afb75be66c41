"""Plain numpy restatement of N3Tree.leaf_neighbors, the edge plan and N3Tree.tv (include/svoxt.h).  It
shares no code with the package: the GPU tests compare the HIP pipeline with it byte for byte, the host tests check it
against hand-made cases and, with `integrity`, against a brute-force search on integer boxes."""
import numpy as np

BLOCK = 256                     # lanes per workgroup of the loss tree: part of the definition


def leaf_slots(child, n):
    """Flat slots of the leaves of nodes < n, ascending: `_all_leaves()` order."""
    return np.nonzero(np.asarray(child)[:n].reshape(-1) == 0)[0]


def cells(child, parent_depth, n, N):
    """(slots [L], depths [L], c int64 [L, 3]): every leaf's depth and integer cell coordinate in [0, N^(d + 1))^3."""
    n3 = N ** 3
    pd = np.asarray(parent_depth).astype(np.int64)
    slots = leaf_slots(child, n)
    node, slot = slots // n3, slots % n3
    depths = pd[node, 1]
    c = np.zeros((len(slots), 3), np.int64)
    mul = np.ones(len(slots), np.int64)
    live = np.ones(len(slots), bool)
    while live.any():
        digits = np.stack((slot // (N * N), (slot // N) % N, slot % N), axis=1)
        c[live] += (digits * mul[:, None])[live]
        live &= node != 0
        packed = pd[np.where(live, node, 0), 0]
        node, slot = np.where(live, packed // n3, 0), np.where(live, packed % n3, slot)
        mul *= N
    return slots, depths, c


def lookup(child, n, N, index, d, t):
    """The descent: for cells t [Q, 3] of level d [Q] the leaf index of the leaf met on the way down, -2 where the cell
    is still a node after level d."""
    n3 = N ** 3
    ch = np.asarray(child)[:n].reshape(-1).astype(np.int64)
    Q = len(d)
    node = np.zeros(Q, np.int64)
    res = np.full(Q, -2, np.int64)
    open_ = np.ones(Q, bool)
    for l in range(int(d.max()) + 1 if Q else 0):
        act = open_ & (l <= d)
        q = N ** np.where(act, d - l, 0)
        dig = (t // q[:, None]) % N
        s = node * n3 + (dig[:, 0] * N + dig[:, 1]) * N + dig[:, 2]
        s = np.where(act, s, 0)
        leaf = act & (ch[s] == 0)
        res[leaf] = index[s[leaf]]
        open_ &= ~leaf
        node = np.where(act & ~leaf, node + ch[s], node)
    return res


def leaf_neighbors(child, parent_depth, n, N):
    """int32 [L, 6]: columns -x +x -y +y -z +z; leaf index of the same-size or coarser neighbour, -1 outside, -2 finer."""
    slots, depths, c = cells(child, parent_depth, n, N)
    index = np.full(n * N ** 3, -1, np.int64)
    index[slots] = np.arange(len(slots))
    out = np.empty((len(slots), 6), np.int32)
    side = N ** (depths + 1)
    for k in range(6):
        t = c.copy()
        t[:, k // 2] += 1 if k % 2 else -1
        inside = (t[:, k // 2] >= 0) & (t[:, k // 2] < side)
        res = lookup(child, n, N, index, depths, np.where(inside[:, None], t, 0))
        out[:, k] = np.where(inside, res, -1)
    return out


def leaf_rows(child, data, n, M):
    """int64 [L]: the row a leaf names (its data word read unsigned, below M), -1 for an empty leaf."""
    words = np.asarray(data)[:n].reshape(-1)[leaf_slots(child, n)].astype(np.int64) & 0xFFFFFFFF
    return np.where(words < M, words, -1)


def edges(neighbors, depths, rows, M):
    """[(e, i, j)] ascending in e = 6 i + k: the slots of the table that are edges."""
    out = []
    for i in range(neighbors.shape[0]):
        for k in range(6):
            j = int(neighbors[i, k])
            if j < 0:
                continue
            if not (depths[j] < depths[i] or (depths[j] == depths[i] and k % 2 == 1)):
                continue
            if not (0 <= rows[i] < M and 0 <= rows[j] < M) or rows[i] == rows[j]:
                continue
            out.append((6 * i + k, i, j))
    return out


def plan(neighbors, depths, rows, M):
    """dict(row_ptr int32 [M + 1], other int32 [2 E], meta uint8 [2 E] = depth_i << 1 | (1 for a - incidence), E)."""
    inc = []                                       # (owner, id, other, meta)
    for e, i, j in edges(neighbors, depths, rows, M):
        inc.append((int(rows[i]), 2 * e, int(rows[j]), int(depths[i]) << 1))
        inc.append((int(rows[j]), 2 * e + 1, int(rows[i]), int(depths[i]) << 1 | 1))
    inc.sort(key=lambda t: (t[0], t[1]))           # by owning row, ascending incidence id within a row
    owners = np.array([t[0] for t in inc], np.int64)
    return dict(row_ptr=np.searchsorted(owners, np.arange(M + 1)).astype(np.int32),
                other=np.array([t[2] for t in inc], np.int32), meta=np.array([t[3] for t in inc], np.uint8), E=len(inc) // 2)


def _tree_sum(v):
    """v[..., i] = v[..., i] + v[..., i + s] for s = 128, 64 .. 1 over the last axis of 256 float32."""
    v = v.copy()
    s = BLOCK // 2
    while s:
        v[..., :s] = v[..., :s] + v[..., s:2 * s]
        s //= 2
    return v[..., 0]


def _padded(a):
    return np.concatenate((a, np.zeros(-len(a) % BLOCK, np.float32))).reshape(-1, BLOCK)


def tv(features, pl, cols, p, weight, N, mean=False):
    """(loss float32, G float32 [M, K]): float32 operation by operation in the documented order.  cols: column indices
    or None for all; weight "uniform" / "area"."""
    f = np.asarray(features, np.float32)
    M, K = f.shape
    cols = np.arange(K) if cols is None else np.asarray(cols, np.int64)
    Kc = len(cols)
    wtab = np.array([float(N) ** (-2 * (d + 1)) for d in range(32)], np.float64).astype(np.float32)
    G = np.zeros((M, K), np.float32)
    lanes = np.zeros((M, Kc), np.float32)
    row_ptr, other, meta = pl["row_ptr"].astype(np.int64), pl["other"], pl["meta"]
    counts = np.diff(row_ptr)
    live = np.nonzero(counts > 0)[0]
    a = f[np.ix_(live, cols)]
    g = np.zeros((len(live), Kc), np.float32)
    l = np.zeros((len(live), Kc), np.float32)
    for s in range(int(counts.max()) if len(live) else 0):          # every row's s-th incidence: per row the order is sequential
        act = np.nonzero(counts[live] > s)[0]
        q = row_ptr[live[act]] + s
        b = f[other[q]][:, cols]
        w = (wtab[meta[q] >> 1] if weight == "area" else np.ones(len(q), np.float32))[:, None]
        diff = a[act] - b
        if p == 2:
            t = w * diff
            g[act] = g[act] + (t + t)
            term = t * diff
        else:
            g[act] = g[act] + np.sign(diff) * w
            term = w * np.abs(diff)
        plus = act[(meta[q] & 1) == 0]                               # the loss counts an edge once: on its + incidence
        l[plus] = l[plus] + term[(meta[q] & 1) == 0]
    assert g.dtype == l.dtype == np.float32
    G[np.ix_(live, cols)] = g
    lanes[live] = l
    loss = np.float32(0)
    if M * Kc > 0 and pl["E"] > 0:
        partials = _tree_sum(_padded(lanes.reshape(-1)))
        acc = np.zeros(BLOCK, np.float32)
        for row in _padded(partials):
            acc = acc + row
        loss = _tree_sum(acc)
    if mean and pl["E"] > 0:
        D = np.float32(pl["E"] * Kc)
        loss, G = np.float32(loss / D), (G / D).astype(np.float32)
    return np.float32(loss), G


def add_grad(out, scale, G, pl, cols):
    """out + scale * G (a multiply, an add, each rounded) at the selected columns of the rows with an incidence."""
    res = np.array(out, np.float32)
    K = res.shape[1]
    cols = np.arange(K) if cols is None else np.asarray(cols, np.int64)
    live = np.nonzero(np.diff(pl["row_ptr"]) > 0)[0]
    at = np.ix_(live, cols)
    res[at] = res[at] + np.float32(scale) * G[at]
    return res


def adjacent_pairs(child, parent_depth, n, N):
    """Brute force on integer boxes: the set of (i, j), i < j, of leaves whose boxes share a piece of a face.  The cube
    is rasterised at the finest level, each fine cell holding its leaf's index."""
    slots, depths, c = cells(child, parent_depth, n, N)
    top = int(depths.max())
    R = N ** (top + 1)
    assert R ** 3 <= 1 << 25, "too fine to rasterise"
    grid = np.full((R, R, R), -1, np.int64)
    for i in range(len(slots)):
        w = N ** (top - int(depths[i]))
        lo = c[i] * w
        grid[lo[0]:lo[0] + w, lo[1]:lo[1] + w, lo[2]:lo[2] + w] = i
    assert (grid >= 0).all()
    pairs = set()
    for axis in range(3):
        a = np.moveaxis(grid, axis, 0)
        x, y = a[:-1].reshape(-1), a[1:].reshape(-1)
        ne = x != y
        pairs |= set(map(tuple, np.unique(np.stack((np.minimum(x, y)[ne], np.maximum(x, y)[ne]), 1), axis=0).tolist()))
    return pairs


def integrity(neighbors, child, parent_depth, n, N):
    """Asserts: equal-depth neighbours are mutual; -1 iff the target lies outside; -2 iff the target cell is a node;
    every pair of face-adjacent leaves (brute force) is in the edge set exactly once."""
    slots, depths, c = cells(child, parent_depth, n, N)
    L = len(slots)
    assert neighbors.shape == (L, 6) and neighbors.dtype == np.int32
    # the cells that are nodes, per level: the set of (level, cell) of every internal slot
    n3 = N ** 3
    pd = np.asarray(parent_depth).astype(np.int64)
    inner = set()
    node_cell = {0: (0, 0, 0)}
    ch = np.asarray(child)[:n].reshape(n, n3)
    for node in range(n):                          # parents come before children
        base = node_cell[node]
        for slot in np.nonzero(ch[node])[0]:
            cell = (base[0] * N + slot // (N * N), base[1] * N + (slot // N) % N, base[2] * N + slot % N)
            inner.add((int(pd[node, 1]),) + tuple(int(v) for v in cell))
            node_cell[node + int(ch[node, slot])] = cell
    for i in range(L):
        for k in range(6):
            t = c[i].copy()
            t[k // 2] += 1 if k % 2 else -1
            j = int(neighbors[i, k])
            outside = t[k // 2] < 0 or t[k // 2] >= N ** (depths[i] + 1)
            assert (j == -1) == outside, (i, k)
            assert (j == -2) == ((int(depths[i]),) + tuple(int(v) for v in t) in inner), (i, k)
            if j >= 0:
                assert depths[j] <= depths[i]
                if depths[j] == depths[i]:
                    assert neighbors[j, k ^ 1] == i, (i, k)
    rows = np.arange(L)                            # a row per leaf: every adjacent pair is an edge
    found = [(min(i, j), max(i, j)) for _, i, j in edges(neighbors, depths, rows, L)]
    assert len(found) == len(set(found))
    assert set(found) == adjacent_pairs(child, parent_depth, n, N)
    return len(found)
