"""Restatement of RaySamples.split and merge_samples (include/svoxt.h, svoxt_samples_split_* / svoxt_samples_merge_*) in
numpy on the CPU: sequential, float32, operation for operation.

TEST INFRASTRUCTURE ONLY; nothing here imports the library.  Ray q's segment is max(offsets[q], 0) .. min(offsets[q + 1], T).
Every +, -, * and / below is one numpy float32 operation on float32 operands: IEEE, one rounding, never fused.

    split(offsets, ray, row, depth, length, max_length=None, pieces=None, max_pieces=4096)
                                             (offsets', ray', row', depth', length', index): for sample k
                                                 mf = ceil(length / max_length)  or  float32(pieces[k])
                                                 m = 1 where length > 0 is false or mf >= 1 is false, else int(min(mf, float32(max_pieces)))
                                                 m == 1: copied;  else step = length / float32(m), piece p: depth + float32(p) * step, step
                                             offsets'[q] = pos[clamped offsets[q]], pos the number of pieces before each sample
    split_counts(length, max_length, pieces, max_pieces)     int64 [T]: m alone
    merge(a, b)                              (Lists m with row = -1, index_a, index_b) for two Lists of the same rays: the walk
                                             of include/svoxt.h, rule by rule (merge_ray below)
    union(a, b)                              [(start, index_a, index_b)] per ray by brute force, for lists whose samples all
                                             have e > s and do not overlap inside a list: all breakpoints of the ray sorted,
                                             coverage decided at each midpoint in float64.  Shares no code with merge.
    alpha_bound(...) / split_alpha_bound(...) the bounds below

THE BOUND ON THE MIXTURE ALPHA.  u = 2^-24.  The float32 side is sample_weights over the merged lists with sigma =
sigma_a + sigma_b (take_samples: 0 where a list has no sample); the float64 side is 1 - (1 - alpha_a)(1 - alpha_b) from the
two lists apart.  In exact arithmetic they agree where the pieces of a sample tile it: T_end = exp(-X) with X = sum over
pieces of length * sigma = sum over the samples of both lists of length * sigma.  Per merged piece with sigma > 0 the
float32 side rounds
    the sum sigma_a + sigma_b, the piece's length (a difference of two cursors, or a copy), the product length * sigma:
        three relative errors u on the exponent x_p = length_p * sigma_p, 3 u x_p on ln T;
    the exponential (priced at two units in the last place, 4 u, relative) and the product T * att (u): 5 u on ln T whatever
        x_p is -- att close to 1 is rounded to a grid of u / 2 however small x_p is, which is why no bound of the form
        "roundings times u times sum length * sigma" alone can hold: a ray of n pieces with X -> 0 still moves alpha by n u / 2.
A cut sample adds a geometric term: its end e = depth + length is one float32 add, off the real s + length by at most
u |e|, so the lengths of its pieces sum to length only within u |e| (plus the differences' own roundings, priced above):
sigma_k u |e_k| on ln T for every sample k of either list.  With T <= 1, |d alpha| <= |d ln T|, and the final 1 - T adds u:

    |alpha32 - alpha64| <= u (5 n + 3 X + G + 1),   n = merged pieces with sigma > 0, X = sum_p length_p sigma_p,
                                                     G = sum over the samples of both lists with sigma > 0 of sigma |depth + length|

(first order in u; the second order is below 1e-6 of it at these sizes).  tests/test_cut_host.py holds the restatement to
half of it, the GPU tests hold the kernels to all of it.

split against the lists it came from, both float32: the unsplit side rounds one product, the exponential and T * att per
sample (u (5 n + X) + u), the split side per piece the quotient length / m, the product and those five (u (5 n' + 2 X) + u;
m * (length / m) is length within u length):

    |alpha32(split) - alpha32| <= u (5 (n + n') + 3 X + 2)

The two are not equal bit for bit: exp(-(length * sigma)) is one rounded exponential, the product of m rounded
exponentials of -(step * sigma) is another number.
"""
from __future__ import annotations

import numpy as np

from tests.samples_restate import Lists

F = np.float32
U = 2.0 ** -24


def segments(offsets, T):
    offsets = np.asarray(offsets, dtype=np.int64)
    return np.maximum(offsets[:-1], 0), np.minimum(offsets[1:], T)


# ---------------------------------------------------------------------------------------------------------------- split
def split_counts(length, max_length=None, pieces=None, max_pieces=4096):
    assert (max_length is None) != (pieces is None)
    length = np.asarray(length, dtype=F)
    with np.errstate(all="ignore"):
        mf = np.ceil(length / F(max_length)).astype(F) if pieces is None else np.asarray(pieces, dtype=np.int32).astype(F)
        cut = (length > 0) & (mf >= 1)
        m = np.minimum(np.where(cut, mf, F(1)), F(max_pieces)).astype(np.int64)
    return np.where(cut, m, 1)


def split(offsets, ray, row, depth, length, max_length=None, pieces=None, max_pieces=4096):
    depth, length = np.asarray(depth, dtype=F), np.asarray(length, dtype=F)
    T = length.shape[0]
    m = split_counts(length, max_length, pieces, max_pieces)
    pos = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    index = np.repeat(np.arange(T, dtype=np.int64), m)
    p = np.arange(int(pos[-1]), dtype=np.int64) - pos[index]
    mi = m[index]
    with np.errstate(all="ignore"):
        step = length[index] / mi.astype(F)
        z = depth[index] + p.astype(F) * step
    whole = mi == 1
    new_depth = np.where(whole, depth[index], z).astype(F)
    new_length = np.where(whole, length[index], step).astype(F)
    # (np.where keeps the bits of the branch it takes, a NaN's payload included)
    new_offsets = pos[np.clip(np.asarray(offsets, dtype=np.int64), 0, T)]
    return new_offsets, np.asarray(ray)[index], np.asarray(row)[index], new_depth, new_length, index


# ---------------------------------------------------------------------------------------------------------------- merge
class _Cursor:
    """One list of a ray under the walk: the current sample [s, e), its length as stored, and the cursor c."""

    def __init__(self, depth, length, k, end):
        self.depth, self.length, self.k, self.end = depth, length, k, end
        self.load()

    def live(self):
        return self.k < self.end

    def load(self):
        if self.k < self.end:
            self.s = self.depth[self.k]
            self.len = self.length[self.k]
            self.e = F(self.s + self.len)
            self.c = self.s

    def next(self):
        self.k += 1
        self.load()

    def rest(self):
        return self.len if self.c == self.s else F(self.e - self.c)


def merge_ray(depth_a, length_a, ka, ea, depth_b, length_b, kb, eb):
    """[(depth, length, index_a, index_b)] of one ray: include/svoxt.h's rules 1 .. 6, the first that applies."""
    a, b = _Cursor(depth_a, length_a, ka, ea), _Cursor(depth_b, length_b, kb, eb)
    out = []
    with np.errstate(all="ignore"):
        while a.live() or b.live():
            if a.live() and not a.e > a.s:                                    # 1
                out.append((a.s, a.len, a.k, -1))
                a.next()
            elif b.live() and not b.e > b.s:
                out.append((b.s, b.len, -1, b.k))
                b.next()
            elif a.live() and (not b.live() or a.e <= b.c):                   # 2
                out.append((a.c, a.rest(), a.k, -1))
                a.next()
            elif not a.live() or b.e <= a.c:                                  # 3
                out.append((b.c, b.rest(), -1, b.k))
                b.next()
            elif a.c < b.c:                                                   # 4
                out.append((a.c, F(b.c - a.c), a.k, -1))
                a.c = b.c
            elif b.c < a.c:                                                   # 5
                out.append((b.c, F(a.c - b.c), -1, b.k))
                b.c = a.c
            else:                                                             # 6
                hi = b.e if b.e < a.e else a.e
                if a.c == a.s and hi == a.e:
                    d = a.len
                elif b.c == b.s and hi == b.e:
                    d = b.len
                else:
                    d = F(hi - a.c)
                out.append((a.c, d, a.k, b.k))
                a_done, b_done = a.e <= hi, b.e <= hi
                a.c = b.c = hi
                if a_done:
                    a.next()
                if b_done:
                    b.next()
    return out


def merge(a: Lists, b: Lists):
    Q = len(a.offsets) - 1
    assert len(b.offsets) - 1 == Q
    da, la = np.asarray(a.depth, dtype=F), np.asarray(a.length, dtype=F)
    db, lb = np.asarray(b.depth, dtype=F), np.asarray(b.length, dtype=F)
    ba, ea = segments(a.offsets, da.shape[0])
    bb, eb = segments(b.offsets, db.shape[0])
    pieces, counts = [], np.zeros(Q, dtype=np.int64)
    for q in range(Q):
        got = merge_ray(da, la, int(ba[q]), int(ea[q]), db, lb, int(bb[q]), int(eb[q]))
        counts[q] = len(got)
        pieces.extend(got)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = len(pieces)
    depth = np.array([p[0] for p in pieces], dtype=F).reshape(n)
    length = np.array([p[1] for p in pieces], dtype=F).reshape(n)
    # (np.array of float32 scalars copies their bits, NaNs included)
    ia = np.array([p[2] for p in pieces], dtype=np.int64).reshape(n)
    ib = np.array([p[3] for p in pieces], dtype=np.int64).reshape(n)
    ray = np.repeat(np.arange(Q), counts).astype(np.int32)
    return Lists(offsets, np.full(n, -1, dtype=np.int32), ray, depth, length), ia, ib


def union(a: Lists, b: Lists):
    """Per ray [(start, index_a, index_b)]: every interval between two neighbouring breakpoints of the ray that a sample
    of either list covers, found by looking at its midpoint.  For samples with e > s that do not overlap inside a list."""
    out = []
    for q in range(len(a.offsets) - 1):
        spans = []
        for L in (a, b):
            ks = range(int(L.offsets[q]), int(L.offsets[q + 1]))
            spans.append([(k, float(L.depth[k]), float(F(L.depth[k] + L.length[k]))) for k in ks])
        cuts = sorted({z for sp in spans for (_, s, e) in sp for z in (s, e)})
        ray = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            mid = 0.5 * (lo + hi)
            who = [next((k for (k, s, e) in sp if s <= mid < e), -1) for sp in spans]
            if who[0] >= 0 or who[1] >= 0:
                ray.append((lo, who[0], who[1]))
        out.append(ray)
    return out


# --------------------------------------------------------------------------------------------------------------- bounds
def _per_ray(offsets, x):
    out = np.zeros(len(offsets) - 1)
    counts = np.diff(np.asarray(offsets, dtype=np.int64))
    np.add.at(out, np.repeat(np.arange(len(counts)), counts), np.asarray(x, dtype=np.float64))
    return out


def alpha_bound(m: Lists, sigma_m, a: Lists, sigma_a, b: Lists, sigma_b):
    """float64 [Q]: u (5 n + 3 X + G + 1) of the docstring."""
    sm = np.asarray(sigma_m, dtype=np.float64)
    live = sm > 0
    n = _per_ray(m.offsets, live)
    X = _per_ray(m.offsets, np.where(live, np.asarray(m.length, dtype=np.float64) * sm, 0.0))
    G = 0.0
    for L, s in ((a, sigma_a), (b, sigma_b)):
        s = np.asarray(s, dtype=np.float64)
        e = np.abs(np.asarray(L.depth, dtype=np.float64) + np.asarray(L.length, dtype=np.float64))
        G = G + _per_ray(L.offsets, np.where(s > 0, s * e, 0.0))
    return U * (5 * n + 3 * X + G + 1)


def split_alpha_bound(s: Lists, sigma, fine_offsets, fine_sigma):
    """float64 [Q]: u (5 (n + n') + 3 X + 2) of the docstring."""
    sg = np.asarray(sigma, dtype=np.float64)
    n = _per_ray(s.offsets, sg > 0)
    n2 = _per_ray(fine_offsets, np.asarray(fine_sigma) > 0)
    X = _per_ray(s.offsets, np.where(sg > 0, np.asarray(s.length, dtype=np.float64) * sg, 0.0))
    return U * (5 * (n + n2) + 3 * X + 2)
