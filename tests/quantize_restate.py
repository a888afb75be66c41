"""quantize_median_cut restated in plain numpy for the quantiser tests: median cut level by level, as the operation is
specified -- split column = the first column with the largest float32 (max - min); order within a segment =
(value with the sign of zero dropped, row index); cut = the middle (unweighted) or the first position whose inclusive
float64 prefix of the weights exceeds half the segment's total (weighted); colour index = the left-to-right order of
the closed segments; colour = the (weighted) float64 mean, rounded once to float32.  Shares no code with the package.

The weighted prefixes are differences of one running float64 sum over the sorted rows: that equals the in-segment
sum whenever the sums are exact in float64, which holds for every weight set the tests use (multiples of 2^-10)."""
from __future__ import annotations

import numpy as np


def quantize(data, weights, order, report=None):
    """-> (colors float32 [2^order, K], color_id_map int32 [M], means float64 [2^order, K], starts int64 [S + 1],
    perm int64 [M]): segment c holds the rows perm[starts[c]:starts[c + 1]]; means is the palette before rounding.

    report: a dict that receives `unique` -- True iff at every split the winning column's range was a strict maximum
    and the values either side of the cut in that column differed (then no tie-break decides anything: any correct
    median cut gives the same color_id_map)."""
    data = np.ascontiguousarray(data, np.float32)
    M, K = data.shape
    weighted = weights is not None and len(weights) > 0
    w = np.asarray(weights, np.float32).astype(np.float64) if weighted else None
    assert 0 <= order <= 16 and (1 << order) <= M and K >= 1
    perm = np.arange(M, dtype=np.int64)
    starts = np.array([0, M], np.int64)
    unique = True
    for _ in range(order):
        lens = np.diff(starts)
        S = len(lens)
        seg = np.repeat(np.arange(S), lens)
        live = lens > 0
        rows = data[perm]
        at = starts[:-1][live]
        mn = np.full((S, K), np.inf, np.float32)
        mx = np.full((S, K), -np.inf, np.float32)
        mn[live] = np.minimum.reduceat(rows, at, axis=0)
        mx[live] = np.maximum.reduceat(rows, at, axis=0)
        is_open = lens > 1
        with np.errstate(invalid="ignore"):
            rng = (mx - mn).astype(np.float32)
        rng[~is_open] = 0
        col = np.argmax(rng, axis=1)                             # the first column with the largest range
        top = rng[np.arange(S), col]
        if K > 1 and ((rng == top[:, None]).sum(axis=1)[is_open] > 1).any():
            unique = False
        val = rows[np.arange(M), col[seg]] + np.float32(0.0)     # -0.0 + 0.0 = +0.0
        val[~is_open[seg]] = 0                                   # closed segments keep their order
        srt = np.lexsort((perm, val, seg))
        perm, val = perm[srt], val[srt]
        l, r = starts[:-1], starts[1:]
        if not weighted:
            m = l + (r - l) // 2
        else:
            run = np.concatenate(([0.0], np.cumsum(w[perm])))
            pre = run[1:] - run[l][seg]                          # inclusive prefix within the segment
            tot = run[r] - run[l]
            pos = np.arange(M)
            first = np.where(pre > 0.5 * tot[seg], pos, r[seg])
            m = r.copy()
            m[live] = np.minimum.reduceat(first, at)
        cut = is_open & (m > l) & (m < r)
        if (val[m[cut] - 1] == val[m[cut]]).any():
            unique = False
        n_out = np.where(is_open, 2, 1)
        slot = np.concatenate(([0], np.cumsum(n_out)))
        new = np.empty(slot[-1] + 1, np.int64)
        new[slot[:-1]] = l
        new[slot[:-1][is_open] + 1] = m[is_open]
        new[-1] = M
        starts = new
    S = len(starts) - 1
    assert S <= 1 << order
    lens = np.diff(starts)
    live = lens > 0
    at = starts[:-1][live]
    seg = np.repeat(np.arange(S), lens)
    rows = data[perm].astype(np.float64)
    means = np.zeros((1 << order, K), np.float64)
    plain = np.add.reduceat(rows, at, axis=0) / lens[live][:, None]
    if weighted:
        ws = w[perm]
        tw = np.add.reduceat(ws, at)
        with np.errstate(invalid="ignore", divide="ignore"):
            wm = np.add.reduceat(rows * ws[:, None], at, axis=0) / tw[:, None]
        means[:S][live] = np.where((tw == 0)[:, None], plain, wm)
    else:
        means[:S][live] = plain
    ids = np.empty(M, np.int32)
    ids[perm] = seg
    if report is not None:
        report["unique"] = unique
    return means.astype(np.float32), ids, means, starts, perm


def reference_bound(data, weights, starts, perm):
    """The float32 sequential-sum bound on every colour entry of the reference's own palette, [S, K] float64:
    (n + 2) 2^-24 sum|w x| / sum w for a segment of n rows (w = 1 unweighted); 0 for an empty segment."""
    data = np.asarray(data, np.float64)
    weighted = weights is not None and len(weights) > 0
    S = len(starts) - 1
    out = np.zeros((S, data.shape[1]), np.float64)
    for c in range(S):
        rows = perm[starts[c]:starts[c + 1]]
        n = len(rows)
        if n == 0:
            continue
        ww = np.asarray(weights, np.float64)[rows] if weighted else np.ones(n)
        out[c] = (n + 2) * 2.0 ** -24 * (np.abs(ww[:, None] * data[rows])).sum(axis=0) / ww.sum()
    return out
