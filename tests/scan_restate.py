"""Restatement of ray_scan, ray_quantile and RaySamples.select (include/svoxt.h, svoxt_ray_scan_* / svoxt_ray_quantile /
svoxt_samples_select_*) in numpy and torch on the CPU.

TEST INFRASTRUCTURE ONLY; nothing here imports the library.  Ray q's segment is max(offsets[q], 0) .. min(offsets[q + 1], T).

    scan(values, offsets, op, exclusive, reverse)             float32 [T, C]: the kernels' sequence.  Every + and * below is
                                                              one numpy float32 operation on float32 operands -- IEEE, one
                                                              rounding, never fused -- done for all rays at once position
                                                              by position, which is the per-ray sequential order:
                                                                  acc = 0 | 1 | -inf | +inf
                                                                  new = acc + v | acc * v | v if v > acc else acc | v if v < acc else acc
                                                                  out = acc if exclusive else new;  acc = new
    scan_backward(values, offsets, op, exclusive, reverse, g) float32 [T, C]: the kernels' backward sequences (below)
    scan64(values, offsets, op, exclusive, reverse)           the same function in torch float64, ray by ray, for autograd
    grad64(values, offsets, op, exclusive, reverse, g)        (gradient, sum of the absolute values of its terms) in float64
    quantile(w, offsets, q, normalize)                        (index int64 [Q, nq], frac float32 [Q, nq])
    select(keep, offsets, ray, row, depth, length)            (offsets', ray', row', depth', length', index)

The float32 backward sequences, positions j = 0 .. n-1 along the scan's direction, g the upstream gradient:
    sum        the scan of g with the same `exclusive` and the other direction
    prod       sweep 1 against the direction:  S_j = g_j + v_{j+1} * S_{j+1},  S_{n-1} = g_{n-1}
               (exclusive:                      S_j = g_{j+1} + v_{j+1} * S_{j+1},  S_{n-1} = 0)
               sweep 2 along it, P = 1:         grad_j = P * S_j;  P = P * v_j
    max / min  one sweep along the direction with the running argument a (none at first) and grad = 0 everywhere:
               inclusive: a moves to j where v_j is taken, then grad_a = grad_a + g_j; exclusive: grad_a = grad_a + g_j
               (nowhere while there is no a), then a moves.

Why prod's two sweeps are the gradient.  Inclusive: out_i = prod_{m <= i} v_m, so
    d/dv_j sum_i g_i out_i = sum_{i >= j} g_i prod_{m <= i, m != j} v_m = (prod_{m < j} v_m) * (g_j + v_{j+1} (g_{j+1} + v_{j+2} (...))),
the second factor being S_j in Horner form and the first the P of sweep 2 before position j.  Exclusive: out_i =
prod_{m < i} v_m does not hold v_j for i <= j, so the bracket starts one position later: g_{j+1} + v_{j+1} (g_{j+2} + ...).
No quotient out / v_j anywhere: a zero among the values costs nothing.

The bound of tests/test_scan_host.py, 2 n 2^-24 sum|terms| with n the longest ray.  A gradient entry is a sum of terms,
each a g_i times values (prod), or a g_i alone (sum, max, min).  In the float32 sequences term i of entry j passes
through at most (i - j) products and (i - j) + 1 sums inside S_j, then j - 1 products inside P and the product P * S_j:
2 (i - j) + j + 1 <= 2 n roundings, each of relative size at most u = 2^-24, so the entry is off by at most
((1 + u)^(2n) - 1) sum|terms| = 2 n u sum|terms| to first order (the second order, 2 n^2 u^2, is 1e-10 of that at
n = 40).  sum and max / min have at most n sums and no product: the same bound with room.  sum|terms| is the float64
gradient of the same function with |g| upstream and, for prod, |v| as values: every term is then its own absolute value.
"""
from __future__ import annotations

import numpy as np
import torch

OPS = ("sum", "prod", "max", "min")
IDENTITY = {"sum": 0.0, "prod": 1.0, "max": -np.inf, "min": np.inf}


def segments(offsets, T):
    offsets = np.asarray(offsets, dtype=np.int64)
    b = np.maximum(offsets[:-1], 0)
    e = np.minimum(offsets[1:], T)
    return b, e, np.maximum(e - b, 0)


def walk(offsets, T, reverse):
    """[(rays, samples)] for position 0, 1, ... along the scan's direction: the rays that have such a sample, and its index."""
    b, e, n = segments(offsets, T)
    out = []
    for j in range(int(n.max()) if n.size else 0):
        r = np.nonzero(n > j)[0]
        out.append((r, e[r] - 1 - j if reverse else b[r] + j))
    return out, n


def _two(values):
    v = np.asarray(values, dtype=np.float32)
    return (v[:, None], True) if v.ndim == 1 else (v, False)


def scan(values, offsets, op, exclusive=False, reverse=False):
    v, flat = _two(values)
    T, C = v.shape
    steps, _ = walk(offsets, T, reverse)
    acc = np.full((len(offsets) - 1, C), IDENTITY[op], dtype=np.float32)
    out = np.zeros((T, C), dtype=np.float32)
    with np.errstate(all="ignore"):
        for r, k in steps:
            a, x = acc[r], v[k]
            if op == "sum":
                new = a + x
            elif op == "prod":
                new = a * x
            elif op == "max":
                new = np.where(x > a, x, a)
            else:
                new = np.where(x < a, x, a)
            out[k] = a if exclusive else new
            acc[r] = new
    assert out.dtype == np.float32
    return out[:, 0] if flat else out


def scan_backward(values, offsets, op, exclusive, reverse, g):
    v, flat = _two(values)
    g, _ = _two(g)
    T, C = v.shape
    Q = len(offsets) - 1
    if op == "sum":
        out = scan(g, offsets, "sum", exclusive, not reverse)
        return out[:, 0] if flat else out
    steps, n = walk(offsets, T, reverse)
    grad = np.zeros((T, C), dtype=np.float32)
    with np.errstate(all="ignore"):
        if op == "prod":
            S = np.zeros((Q, C), dtype=np.float32)
            v_next = np.zeros((Q, C), dtype=np.float32)
            g_next = np.zeros((Q, C), dtype=np.float32)
            for j in range(len(steps) - 1, -1, -1):
                r, k = steps[j]
                last = (n[r] - 1 == j)[:, None]
                s_last = np.zeros_like(g[k]) if exclusive else g[k]
                s_inner = (g_next[r] if exclusive else g[k]) + v_next[r] * S[r]
                s = np.where(last, s_last, s_inner).astype(np.float32)
                grad[k] = s
                S[r], v_next[r], g_next[r] = s, v[k], g[k]
            P = np.ones((Q, C), dtype=np.float32)
            for r, k in steps:
                grad[k] = P[r] * grad[k]
                P[r] = P[r] * v[k]
        else:
            acc = np.full((Q, C), IDENTITY[op], dtype=np.float32)
            arg = np.full((Q, C), -1, dtype=np.int64)
            cols = np.broadcast_to(np.arange(C), (Q, C))

            def add(r, k):
                a, m = arg[r], arg[r] >= 0
                grad[a[m], cols[r][m]] = grad[a[m], cols[r][m]] + g[k][m]

            for r, k in steps:
                if exclusive:
                    add(r, k)
                take = v[k] > acc[r] if op == "max" else v[k] < acc[r]
                arg[r] = np.where(take, k[:, None], arg[r])
                acc[r] = np.where(take, v[k], acc[r])
                if not exclusive:
                    add(r, k)
    assert grad.dtype == np.float32
    return grad[:, 0] if flat else grad


def scan64(values, offsets, op, exclusive=False, reverse=False):
    """torch float64 [T, C], differentiable in `values` (a float64 tensor [T, C])."""
    T, C = values.shape
    b, e, _ = segments(offsets, T)
    rows = [None] * T
    for q in range(len(offsets) - 1):
        acc = torch.full((C,), IDENTITY[op], dtype=torch.float64)
        ks = range(int(b[q]), int(e[q]))
        for k in (reversed(ks) if reverse else ks):
            x = values[k]
            if op == "sum":
                new = acc + x
            elif op == "prod":
                new = acc * x
            elif op == "max":
                new = torch.where(x > acc, x, acc)
            else:
                new = torch.where(x < acc, x, acc)
            rows[k] = acc if exclusive else new
            acc = new
    zero = torch.zeros((C,), dtype=torch.float64)
    return torch.stack([zero if x is None else x for x in rows]) if T else values.new_zeros((0, C))


def grad64(values, offsets, op, exclusive, reverse, g):
    """(gradient, sum of the absolute values of its terms), float64 numpy [T, C]."""
    out = []
    for vv, gg in ((values, g), (np.abs(values) if op == "prod" else values, np.abs(g))):
        x = torch.from_numpy(np.asarray(vv, dtype=np.float64)).requires_grad_(True)
        y = scan64(x, offsets, op, exclusive, reverse)
        live = torch.isfinite(y.detach())                      # (a position that wrote max's / min's identity takes no gradient)
        (torch.where(live, y, torch.zeros_like(y)) * torch.from_numpy(np.asarray(gg, dtype=np.float64))).sum().backward()
        out.append(x.grad.numpy())
    return out[0], out[1]


def quantile(w, offsets, q, normalize=True):
    w = np.asarray(w, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32).reshape(-1)
    T, Q = w.shape[0], len(offsets) - 1
    b, e, _ = segments(offsets, T)
    index = np.full((Q, q.shape[0]), -1, dtype=np.int64)
    frac = np.zeros((Q, q.shape[0]), dtype=np.float32)
    zero, one = np.float32(0), np.float32(1)
    with np.errstate(all="ignore"):
        for r in range(Q):
            ks, before, after = [], [], []
            c = zero
            for k in range(int(b[r]), int(e[r])):
                if w[k] > 0:
                    ks.append(k)
                    before.append(c)
                    c = np.float32(c + w[k])
                    after.append(c)
            if not ks:
                continue
            after, before = np.asarray(after, dtype=np.float32), np.asarray(before, dtype=np.float32)
            for i, qi in enumerate(q):
                target = np.float32(qi * c) if normalize else qi
                hit = np.nonzero(after >= target)[0]
                if hit.size:
                    j = int(hit[0])
                    f = np.float32(np.float32(target - before[j]) / w[ks[j]])
                    index[r, i] = ks[j]
                    frac[r, i] = zero if not f > 0 else (one if f > 1 else f)
    return index, frac


def select(keep, offsets, ray, row, depth, length):
    keep = np.asarray(keep, dtype=bool)
    T = keep.shape[0]
    pos = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)          # the kept samples before each, T + 1 entries
    index = np.nonzero(keep)[0].astype(np.int64)
    new_offsets = pos[np.clip(np.asarray(offsets, dtype=np.int64), 0, T)]
    return new_offsets, ray[index], row[index], depth[index], length[index], index
