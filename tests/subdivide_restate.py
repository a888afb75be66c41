"""N3Tree.subdivide and N3Tree.unshare restated in plain numpy for the subdivide tests -- the rules as the operations are
specified (which slots split, the new nodes in slot order, the rows behind the old ones) -- and `integrity`, which checks
what the tables of a grown tree must satisfy.  Shares no code with the package."""
from __future__ import annotations

import numpy as np

EMPTY_INDEX = 1410065408          # int(1e10) as int32: the reference's fill value of `data` (svox_t/svox.py:124)


def _is_row(words, M):
    """A data word names a feature row iff, read as an unsigned 32-bit number, it is < M."""
    return (np.asarray(words).astype(np.int64) & 0xFFFFFFFF) < M


def _selected(shape, n, n3, sel, weights, threshold):
    assert sel is None or weights is None
    if sel is not None:
        return np.asarray(sel)[:n].reshape(n, n3) != 0
    if weights is not None:
        with np.errstate(invalid="ignore"):
            return np.asarray(weights, np.float32)[:n].reshape(n, n3) >= np.float32(threshold)       # NaN: never
    return np.ones((n, n3), bool)


def subdivide(child, data, parent_depth, n, M, sel=None, weights=None, threshold=None, depth_limit=10, max_depth=None,
              split_empty=False, own_rows=True, capacity=None):
    """-> (child [cap', N, N, N], data [cap', N, N, N, 1], parent_depth [cap', 2], nodes_added, rows_added,
    row_map int64 [M + rows_added] or None); cap' = `capacity` (default: as little as holds the tree, at least the
    capacity given); rows behind the tree look like unused rows of an N3Tree unless the input's did not."""
    child = np.asarray(child)
    cap, N = child.shape[0], child.shape[1]
    n3 = N ** 3
    limit = depth_limit if max_depth is None else min(depth_limit, max_depth)
    ch = child.reshape(cap, n3).astype(np.int64)
    da = np.asarray(data).reshape(cap, n3).astype(np.int64) & 0xFFFFFFFF
    pd = np.asarray(parent_depth).astype(np.int64)
    full = _is_row(da[:n], M)
    split = (ch[:n] == 0) & _selected(child.shape, n, n3, sel, weights, threshold) & (pd[:n, 1] < limit)[:, None]
    if not split_empty:
        split &= full
    node, slot = np.nonzero(split)                      # ascending flat slot order
    added = node.size
    rows_cap = max(cap, n + added) if capacity is None else capacity
    assert rows_cap >= n + added
    ch2 = np.zeros((rows_cap, n3), np.int64)
    da2 = np.full((rows_cap, n3), EMPTY_INDEX, np.int64)
    pd2 = np.zeros((rows_cap, 2), np.int64)
    ch2[:cap], da2[:cap], pd2[:cap] = ch, da, pd
    new_id = n + np.arange(added)
    ch2[node, slot] = new_id - node
    ch2[new_id] = 0
    pd2[new_id, 0] = node * n3 + slot
    pd2[new_id, 1] = pd[node, 1] + 1
    word = da[node, slot]
    row_map, rows_added = None, 0
    if not own_rows:
        da2[new_id] = word[:, None]
    else:
        brings = full[node, slot]
        k = np.cumsum(brings) - 1
        fresh = M + k[:, None] * (n3 - 1) + np.arange(n3 - 1)[None, :]
        rows = np.concatenate([word[:, None], fresh], axis=1)
        rows[~brings] = EMPTY_INDEX
        da2[new_id] = rows
        rows_added = int(brings.sum()) * (n3 - 1)
        row_map = np.concatenate([np.arange(M), np.repeat(word[brings], n3 - 1)]).astype(np.int64)
    return (ch2.astype(np.int32).reshape(rows_cap, N, N, N), da2.astype(np.uint32).view(np.int32).reshape(rows_cap, N, N, N, 1),
            pd2.astype(np.int32), added, rows_added, row_map)


def unshare(child, data, n, M):
    """-> (data with the shape given, rows_added, row_map int64 [M + rows_added])."""
    child = np.asarray(child)
    cap, N = child.shape[0], child.shape[1]
    n3 = N ** 3
    da = np.asarray(data).reshape(-1).astype(np.int64) & 0xFFFFFFFF
    names = np.zeros(cap * n3, bool)
    names[:n * n3] = (child.reshape(-1)[:n * n3] == 0) & _is_row(da[:n * n3], M)
    at = np.nonzero(names)[0]
    seen = np.zeros(M, bool)
    later = np.zeros(at.size, bool)
    for i, s in enumerate(at):                          # the first slot of a row, in flat slot order, keeps it
        later[i] = seen[da[s]]
        seen[da[s]] = True
    move = at[later]
    row_map = np.concatenate([np.arange(M), da[move]]).astype(np.int64)
    da[move] = M + np.arange(move.size)
    return da.astype(np.uint32).view(np.int32).reshape(np.asarray(data).shape), int(move.size), row_map


def integrity(child, data, parent_depth, n, N, M, n_before=None, own_rows=False, row_map=None, M_before=None):
    """Raises AssertionError unless: every node but the root is reached from exactly one parent slot, whose child
    offset points at it and which its parent_depth[:, 0] points back to; depth = the parent's + 1; every leaf word is a
    row < M or empty.  With `n_before`: the nodes behind it are all-leaf nodes hanging off older nodes; with
    `own_rows` no row is named twice among their leaves (nor by an older leaf); with `row_map`: [:M_before] is arange
    and every entry an old row."""
    n3 = N ** 3
    ch = np.asarray(child)[:n].reshape(n, n3).astype(np.int64)
    da = np.asarray(data)[:n].reshape(n, n3).astype(np.int64) & 0xFFFFFFFF
    pd = np.asarray(parent_depth)[:n].astype(np.int64)
    assert n >= 1 and tuple(pd[0]) == (0, 0)
    node, slot = np.nonzero(ch)
    kid = node + ch[node, slot]
    assert ((kid >= 1) & (kid < n)).all()
    assert (np.bincount(kid, minlength=n) == np.r_[0, np.ones(n - 1, np.int64)]).all()
    assert (pd[kid, 0] == node * n3 + slot).all()
    assert (pd[kid, 1] == pd[node, 1] + 1).all()
    assert (pd[1:, 1] >= 1).all()
    leaf = ch == 0
    assert (_is_row(da, M) | (da == EMPTY_INDEX))[leaf].all()
    if n_before is not None:
        assert not ch[n_before:].any()
        assert (pd[n_before:, 0] // n3 < n_before).all() and (np.diff(pd[n_before:, 0]) > 0).all()
        if own_rows:
            # no row is named twice among the new leaves: the rows behind M_before once each, all of them, and never by
            # an older leaf; an old row only at slot 0, the one the split leaf named (two split leaves that shared a
            # row still share it there: unshare() is what separates those)
            new = da[n_before:]
            fresh = new[(new >= M_before) & (new < M)]
            assert (np.sort(fresh) == np.arange(M_before, M)).all()
            assert not (_is_row(new[:, 1:], M_before)).any()
            split_word = da.reshape(-1)[pd[n_before:, 0]]
            assert (new[:, 0] == np.where(_is_row(split_word, M_before), split_word, EMPTY_INDEX)).all()
            older = da[:n_before][leaf[:n_before]]
            assert not ((older >= M_before) & (older < M)).any()
    if row_map is not None:
        row_map = np.asarray(row_map)
        assert row_map.dtype == np.int64 and row_map.shape == (M,)
        assert (row_map[:M_before] == np.arange(M_before)).all()
        assert ((row_map >= 0) & (row_map < M_before)).all()
