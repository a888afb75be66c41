"""A plain numpy restatement of the row plan and of reduce_rows (include/svoxt.h, "samples to feature rows and back"):
the plan from a stable argsort of the clamped key and a searchsorted, the reductions as float32 loops in the order the
header defines.  Slow and obvious on purpose; tests compare the GPU's bits against it."""
from collections import namedtuple

import numpy as np

CHUNK = 256
Plan = namedtuple("Plan", "row_ptr perm n_outside longest")


def plan(row, M):
    """row int32 [T] -> Plan: key = row where 0 <= row < M, M for anything else; perm = the stable sort by key."""
    row = np.asarray(row).astype(np.int64)
    key = np.where((row >= 0) & (row < M), row, M)
    perm = np.argsort(key, kind="stable").astype(np.int32)
    row_ptr = np.searchsorted(key[perm], np.arange(M + 1), side="left").astype(np.int32)
    counts = np.diff(row_ptr)
    return Plan(row_ptr, perm, int(row.shape[0] - row_ptr[M]), int(counts.max()) if M > 0 else 0)


def _sum_chunked(v):
    """v float32 [n, C], n >= 1, in sample order: per chunk of 256 ((0 + v_0) + v_1) + ..., then (p_0 + p_1) + p_2 ..."""
    partials = []
    for b in range(0, v.shape[0], CHUNK):
        p = np.zeros(v.shape[1], np.float32)
        for x in v[b:b + CHUNK]:
            p = (p + x).astype(np.float32)
        partials.append(p)
    acc = partials[0]
    for p in partials[1:]:
        acc = (acc + p).astype(np.float32)
    return acc


def sum_sequential(v):
    """The plain sequential float32 sum of v [n, C] from 0: what the chunk rule is NOT beyond 256 samples."""
    acc = np.zeros(v.shape[1], np.float32)
    for x in v:
        acc = (acc + x).astype(np.float32)
    return acc


def reduce(values, row, M, op="sum", empty=0.0):
    """out float32 [M, C] ([M] for 1-D values): the header's reduction of values [T, C] by row."""
    values = np.asarray(values, np.float32)
    flat = values.ndim == 1
    v = values[:, None] if flat else values
    P = plan(row, M)
    out = np.full((M, v.shape[1]), np.float32(empty), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(M):
            ks = P.perm[P.row_ptr[r]:P.row_ptr[r + 1]]
            n = ks.shape[0]
            if n == 0:
                continue
            x = v[ks]
            if op == "sum":
                out[r] = _sum_chunked(x)
            elif op == "mean":
                out[r] = (_sum_chunked(x) / np.float32(n)).astype(np.float32)
            elif op in ("max", "min"):
                best = x.max(axis=0) if op == "max" else x.min(axis=0)           # (numpy's max / min propagate NaN)
                out[r] = np.where(np.isnan(x).any(axis=0), np.float32(np.nan), best)
            else:
                raise ValueError(op)
    return out[:, 0] if flat else out


def gather(table, row, cols=None):
    """out[k, j] = table[row[k], cols[j]], zeros where row[k] is outside [0, M)."""
    table = np.asarray(table, np.float32)
    row = np.asarray(row).astype(np.int64)
    M = table.shape[0]
    inside = (row >= 0) & (row < M)
    t = table if cols is None else table[:, np.asarray(cols)]
    out = np.zeros((row.shape[0], t.shape[1]), np.float32)
    out[inside] = t[row[inside]]
    return out


def gather_grad(g, row, M, K, cols=None):
    """The gradient of gather with respect to the table: [M, K], the chunked sums at the selected columns, 0 elsewhere."""
    s = reduce(g, row, M, "sum", 0.0)
    if cols is None:
        return s
    out = np.zeros((M, K), np.float32)
    out[:, np.asarray(cols)] = s
    return out


def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-24: |float32 sum of n terms - exact| <= gamma_n sum |v|, in any order."""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def hand_made(seed=3):
    """T = 5000, M = 37: rows with 0, 1, 255, 256, 257, 512, 513 and 1500 samples, row 0 unused, row M - 1 used, entries
    of -1, M and 2^31 - 1; shuffled."""
    rng = np.random.default_rng(seed)
    M, T = 37, 5000
    sizes = {1: 1, 2: 255, 3: 256, 4: 257, 5: 512, 6: 513, 7: 1500, M - 1: 300}
    row = np.concatenate([np.full(n, r, np.int64) for r, n in sizes.items()])
    outside = np.array([-1] * 5 + [M] * 4 + [2 ** 31 - 1] * 3 + [-2 ** 31], np.int64)
    rest = T - row.shape[0] - outside.shape[0]
    filler = rng.integers(9, M - 1, rest)                               # rows 9 .. M - 2, about 50 each; 0 and 8 stay unused
    row = np.concatenate([row, outside, filler])
    rng.shuffle(row)
    return row.astype(np.int32), M, sizes
