"""N3Tree.set restated in numpy: which row every point writes, the groups, the reductions.

The leaf of a point is the CPU oracle's point query (oracle.query: the yardstick of query_vertical).  The rest is
restated here, in the order DESIGN.md 4.13 documents:
  - a point whose leaf names no row (data word outside [0, M)) is ignored;
  - the other points are grouped by ROW (slots that share a row form one group);
  - "last": the row takes the values of the group's highest point index;
  - "sum": acc = values[q0]; acc = acc + values[q] for the group's points in ASCENDING POINT INDEX, one float32
    addition at a time per column; "mean": that sum divided once by float32(count);
  - "max" / "min": acc = values[q0]; then x > acc ? x : acc (x < acc) in the same order;
  - rows without a point are untouched.
"""
import numpy as np

from oracle import oracle as O

MODES = ("last", "sum", "mean", "max", "min")


def point_rows(child, data, M, points, offset=(0, 0, 0), scaling=(1, 1, 1)):
    """int64 [Q]: the feature row of every point's leaf, -1 where the leaf is empty (the oracle's point query)."""
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    if points.shape[0] == 0:
        return np.zeros((0,), np.int64)
    t = O.Tree(np.zeros((int(M), 1), np.float32), np.asarray(data), np.asarray(child), offset=offset, scaling=scaling)
    return O.query(t, points)[2].astype(np.int64)


def groups(rows):
    """(touched rows ascending int64 [U], counts int64 [U], order int64 [P], starts int64 [U + 1]): order lists the
    non-ignored points by (row, point index); group u is order[starts[u]:starts[u + 1]], ascending point indices."""
    rows = np.asarray(rows, np.int64)
    pts = np.nonzero(rows >= 0)[0]
    order = pts[np.argsort(rows[pts], kind="stable")]                # stable: ascending point index within a row
    uniq, first, counts = np.unique(rows[order], return_index=True, return_counts=True)
    return uniq, counts.astype(np.int64), order, np.append(first, order.shape[0]).astype(np.int64)


def reduce_group(vals, mode):
    """One group's rows vals [n, K] float32, in ascending point index -> the row written, float32 [K]; sequential."""
    vals = np.asarray(vals, np.float32)
    if mode == "last":
        return vals[-1].copy()
    acc = vals[0].copy()
    for x in vals[1:]:
        if mode in ("sum", "mean"):
            acc = (acc + x).astype(np.float32)
        elif mode == "max":
            acc = np.where(x > acc, x, acc)
        elif mode == "min":
            acc = np.where(x < acc, x, acc)
        else:
            raise ValueError(mode)
    if mode == "mean":
        acc = (acc / np.float32(vals.shape[0])).astype(np.float32)
    return acc.astype(np.float32)


def assign(table, rows, values, mode, only_rows=None):
    """The table after set(): a copy of table [M, K] with every touched row (or those of only_rows) replaced."""
    out = np.array(table, np.float32, copy=True)
    values = np.asarray(values, np.float32)
    uniq, _, order, starts = groups(rows)
    pick = range(len(uniq)) if only_rows is None else np.nonzero(np.isin(uniq, only_rows))[0]
    for u in pick:
        out[uniq[u]] = reduce_group(values[order[starts[u]:starts[u + 1]]], mode)
    return out


def assign_last(table, rows, values):
    """"last", vectorised (exact: no arithmetic): the highest point index of every row wins."""
    out = np.array(table, np.float32, copy=True)
    rows = np.asarray(rows, np.int64)
    winner = np.full(out.shape[0], -1, np.int64)
    pts = np.nonzero(rows >= 0)[0]
    np.maximum.at(winner, rows[pts], pts)
    hit = winner >= 0
    out[hit] = np.asarray(values, np.float32)[winner[hit]]
    return out
