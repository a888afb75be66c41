"""N3Tree.prune restated in plain numpy for the prune tests -- the four steps as the operation is specified (drop,
collapse level by level from the deepest nodes up, renumber the nodes with a cumulative sum, renumber the feature
rows) -- and `integrity`, which checks what every tree table must satisfy.  Shares no code with the package."""
from __future__ import annotations

import numpy as np

EMPTY_INDEX = 1410065408          # int(1e10) as int32: the reference's fill value of `data` (svox_t/svox.py:124)


def _is_row(words, M):
    """A data word names a feature row iff, read as an unsigned 32-bit number, it is < M."""
    return (np.asarray(words).astype(np.int64) & 0xFFFFFFFF) < M


def prune(child, data, parent_depth, n, M, keep=None, weights=None, threshold=None, collapse=True,
          compact_features=True, reserve=0):
    """-> (child [n' + reserve, N, N, N], data [n' + reserve, N, N, N, 1], parent_depth [n' + reserve, 2], n',
    row_map int64 [M'] or None, leaves dropped)."""
    assert (keep is None) != (weights is None)
    child = np.asarray(child)
    N = child.shape[1]
    n3 = N ** 3
    ch = child[:n].reshape(n, n3).astype(np.int64)
    da = np.asarray(data)[:n].reshape(n, n3).astype(np.int64)
    pd = np.asarray(parent_depth)[:n].astype(np.int64)
    if keep is not None:
        kept = np.asarray(keep)[:n].reshape(n, n3) != 0
    else:
        with np.errstate(invalid="ignore"):
            kept = np.asarray(weights, np.float32)[:n].reshape(n, n3) >= np.float32(threshold)     # NaN: dropped
    leaf = ch == 0
    full = leaf & _is_row(da, M)

    # 1. drop
    drop = full & ~kept
    da[drop] = EMPTY_INDEX
    full &= kept

    # 2. collapse: a node stays iff a full leaf lies below it; decided level by level, the deepest nodes first
    stays = np.ones(n, bool)
    if collapse:
        below = full.any(1)
        depth = pd[:, 1]
        for d in range(int(depth.max()), 0, -1):
            at = np.nonzero(depth == d)[0]            # their own children (depth d + 1) have reported already
            np.logical_or.at(below, pd[at, 0] // n3, below[at])
        stays = below.copy()
        stays[0] = True
        node, slot = np.nonzero(~leaf)
        gone = ~stays[node + ch[node, slot]]
        ch[node[gone], slot[gone]] = 0
        da[node[gone], slot[gone]] = EMPTY_INDEX

    # 3. compact the nodes
    new_id = np.cumsum(stays) - 1
    n_new = int(stays.sum())
    node, slot = np.nonzero(ch)
    ch[node, slot] = new_id[node + ch[node, slot]] - new_id[node]
    da[node, slot] = EMPTY_INDEX                      # inner slots: no stale index
    up, at = pd[:, 0] // n3, pd[:, 0] % n3
    pd[1:, 0] = new_id[up[1:]] * n3 + at[1:]          # the root's row is carried as it is
    ch, da, pd = ch[stays], da[stays], pd[stays]

    # 4. compact the features
    row_map = None
    if compact_features:
        full = (ch == 0) & _is_row(da, M)
        used = np.zeros(M, bool)
        used[da[full]] = True
        row_map = np.nonzero(used)[0].astype(np.int64)
        da[full] = (np.cumsum(used) - 1)[da[full]]

    rows = n_new + reserve
    child_out = np.zeros((rows, N, N, N), np.int32)
    data_out = np.full((rows, N, N, N, 1), EMPTY_INDEX, np.int32)
    pd_out = np.zeros((rows, 2), np.int32)
    child_out[:n_new] = ch.reshape(n_new, N, N, N)
    data_out[:n_new] = (da & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(n_new, N, N, N, 1)
    pd_out[:n_new] = pd
    return child_out, data_out, pd_out, n_new, row_map, int(drop.sum())


def integrity(child, data, parent_depth, n, N, M, collapsed=True, pruned=True):
    """Raises AssertionError unless: every node but the root is reached from exactly one parent slot and the root from
    none; child offsets and parent_depth[:, 0] agree; depth = the parent's + 1 (so there is no cycle and every node
    hangs off the root); every leaf word is a row < M or the empty index; after a prune inner slots hold the empty
    index, and after a collapsing one no node but the root consists of empty leaves alone."""
    n3 = N ** 3
    ch = np.asarray(child)[:n].reshape(n, n3).astype(np.int64)
    da = np.asarray(data)[:n].reshape(n, n3).astype(np.int64)
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
    if pruned:
        assert (da[~leaf] == EMPTY_INDEX).all()
    if collapsed:
        assert (~leaf | _is_row(da, M))[1:].any(1).all()


def number_leaves(child, n, rng, empty=0.2, shared=0.2):
    """A data table for topology that comes without one: leaves get consecutive rows in slot order, except that a
    fraction stays empty and a fraction shares the row of an earlier leaf.  -> (data [n, N, N, N, 1] int32, M)."""
    child = np.asarray(child)[:n]
    leaf = np.nonzero(child.reshape(-1) == 0)[0]
    kind = rng.random(leaf.size)
    kind[0] = 1.0                                     # the first leaf owns row 0
    own = kind >= empty + shared
    rows = np.cumsum(own) - 1                         # for a leaf without a row of its own: the last row before it
    share = (kind >= empty) & ~own
    rows[share] = rng.integers(0, rows[share] + 1)
    data = np.full(child.size, EMPTY_INDEX, np.int32)
    data[leaf[kind >= empty]] = rows[kind >= empty]
    return data.reshape(child.shape + (1,)), int(own.sum())
