"""N3Tree.frontier / reduce_frontier / diam_frontier / merge restated in plain numpy for the merge tests, as the
operations are specified: the frontier by a test per node, the reductions child by child in slot order (float32,
sequential), the diameter in float64, merge by rewriting the tables node by node and renumbering with cumulative sums.
Shares no code with the package."""
from __future__ import annotations

import numpy as np

EMPTY_INDEX = 1410065408          # int(1e10) as int32: the reference's fill value of `data` (svox_t/svox.py:124)


def _u(words):
    return np.asarray(words).astype(np.int64) & 0xFFFFFFFF


def frontier(child, n):
    """int64 [F], ascending: the nodes other than the root whose slots are all leaves."""
    ch = np.asarray(child)[:n].reshape(n, -1)
    sel = (ch == 0).all(1)
    sel[0] = False
    return np.nonzero(sel)[0].astype(np.int64)


def _rows(features, data, n, nodes, cols):
    """x float32 [F, N^3, K'] (zeros at empty children), has bool [F, N^3]."""
    features = np.asarray(features, np.float32)
    M = features.shape[0]
    words = _u(np.asarray(data)[:n].reshape(n, -1)[nodes])
    has = words < M
    x = np.zeros(words.shape + (features.shape[1],), np.float32)
    x[has] = features[words[has]]
    if cols is not None:
        x = x[..., np.atleast_1d(np.asarray(cols))]
    return x, has


def reduce(features, data, n, nodes, op="mean", cols=None, empty="zero"):
    """float32 [F, K']: slots 0 .. N^3 - 1 in order, sequential float32; max / min keep the first slot that attains
    the extremum (a strict comparison replaces).  -> (values, argslot int [F, K'] or None, count int [F])."""
    x, has = _rows(features, data, n, nodes, cols)
    F, n3, Kc = x.shape
    out = np.zeros((F, Kc), np.float32)
    arg = np.full((F, Kc), -1, np.int64)
    count = np.zeros(F, np.int64)
    started = np.zeros(F, bool)
    for c in range(n3):
        use = has[:, c] if empty == "skip" else np.ones(F, bool)
        xc = x[:, c]
        first = use & ~started
        later = use & started
        if op in ("sum", "mean"):
            out[first] = xc[first]
            out[later] = (out[later] + xc[later]).astype(np.float32)
        else:
            with np.errstate(invalid="ignore"):
                better = (xc > out) if op == "max" else (xc < out)
            take = first[:, None] | (later[:, None] & better)
            out[take] = xc[take]
            arg[take] = c
        count += use
        started |= use
    if op == "mean":
        nz = count > 0
        out[nz] = (out[nz] / count[nz, None].astype(np.float32)).astype(np.float32)
    return out, (arg if op in ("max", "min") else None), count


def diam(features, data, n, nodes, cols=None, empty="zero", scale=1.0):
    """float64 [F]: max over pairs of children of ||(x_a - x_b) * scale||, in float64 from the float32 rows."""
    x, has = _rows(features, data, n, nodes, cols)
    x = x.astype(np.float64)
    F, n3, _ = x.shape
    best = np.zeros(F)
    for a in range(n3):
        for b in range(a + 1, n3):
            d = (((x[:, a] - x[:, b]) * float(scale)) ** 2).sum(-1)
            if empty == "skip":
                d = np.where(has[:, a] & has[:, b], d, 0.0)
            best = np.maximum(best, d)
    return np.sqrt(best)


def merge(child, data, parent_depth, n, features, selected_nodes, op="mean", empty="zero", compact_features=True, reserve=0):
    """selected_nodes: ids of the nodes to merge (those that are not frontier nodes are ignored).
    -> (child [n' + reserve, N, N, N], data [n' + reserve, N, N, N, 1], parent_depth [n' + reserve, 2], n',
    features [carried + added, K], row_map int64 [carried] or None, added)."""
    child = np.asarray(child)
    N = child.shape[1]
    n3 = N ** 3
    features = np.asarray(features, np.float32)
    M = features.shape[0]
    ch = child[:n].reshape(n, n3).astype(np.int64)
    da = _u(np.asarray(data)[:n].reshape(n, n3))
    pd = np.asarray(parent_depth)[:n].astype(np.int64)
    front = set(frontier(child, n).tolist())
    merged = np.array(sorted(set(int(i) for i in np.asarray(selected_nodes).reshape(-1)) & front), np.int64)

    # the word each merged node leaves in its parent slot; NEW marks a new row, numbered afterwards
    NEW = -1
    w = da[merged]
    takes_word = (w == w[:, :1]).all(1) | (w >= M).all(1)
    word_of = np.zeros(n, np.int64)
    word_of[merged] = np.where(takes_word, w[:, 0], NEW)
    new_nodes = merged[~takes_word]

    stays = np.ones(n, bool)
    stays[merged] = False
    # old rows carried
    row_map = None
    if compact_features:
        used = np.zeros(M, bool)
        leafw = da[stays][(ch[stays] == 0)]
        used[leafw[leafw < M]] = True
        kept_words = word_of[merged][takes_word]
        used[kept_words[kept_words < M]] = True
        row_map = np.nonzero(used)[0].astype(np.int64)
        renum = np.cumsum(used) - 1
        carried = int(used.sum())
    else:
        renum = np.arange(M)
        carried = M
    new_row_of = np.zeros(n, np.int64)
    new_row_of[new_nodes] = carried + np.arange(len(new_nodes))
    renumbered = lambda w: np.where(w < M, renum[np.minimum(w, max(M - 1, 0))] if M else w, w)      # noqa: E731

    new_id = np.cumsum(stays) - 1
    out_ch = np.zeros((n, n3), np.int64)
    out_da = np.full((n, n3), EMPTY_INDEX, np.int64)
    leaf = ch == 0
    out_da[leaf] = renumbered(da[leaf])
    node, slot = np.nonzero(ch)
    kid = node + ch[node, slot]
    st = stays[kid]
    out_ch[node[st], slot[st]] = new_id[kid[st]] - new_id[node[st]]
    node, slot, kid = node[~st], slot[~st], kid[~st]                 # slots whose child was merged: leaves now
    w = word_of[kid]
    out_da[node, slot] = np.where(w == NEW, new_row_of[kid], renumbered(np.maximum(w, 0)))
    up, at = pd[:, 0] // n3, pd[:, 0] % n3
    out_pd = pd.copy()
    out_pd[1:, 0] = new_id[up[1:]] * n3 + at[1:]
    n_new = int(stays.sum())

    new_rows = reduce(features, data, n, new_nodes, op=op, empty=empty)[0] if len(new_nodes) else np.zeros((0, features.shape[1]), np.float32)
    table = np.concatenate([features[row_map] if compact_features else features, new_rows]).astype(np.float32)

    rows = n_new + reserve
    child_out = np.zeros((rows, N, N, N), np.int32)
    data_out = np.full((rows, N, N, N, 1), EMPTY_INDEX, np.int32)
    pd_out = np.zeros((rows, 2), np.int32)
    child_out[:n_new] = out_ch[stays].reshape(n_new, N, N, N)
    data_out[:n_new] = out_da[stays].astype(np.uint32).view(np.int32).reshape(n_new, N, N, N, 1)
    pd_out[:n_new] = out_pd[stays]
    return child_out, data_out, pd_out, n_new, table, row_map, len(new_nodes)
