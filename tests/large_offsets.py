"""Inputs and exact references for arrays of more than 2^32 elements (tests/test_gpu_large_offsets.py; checked on the host
by tests/test_large_offsets_host.py).  Plain torch and numpy, any device, no kernel of the package.

Everything is a closed-form function of the ABSOLUTE row, sample or ray index, so a 16 GiB input is generated -- and
generated again for the comparison -- a chunk at a time and never kept twice.

Why the comparisons are equalities.  Every value below is a small integer, and next to each pattern stands the largest
sum of absolute values any output element can see.  `assert_exact` checks that it is below 2^24: then every partial sum
of every order of addition is an integer below 2^24 in magnitude, float32 holds each of them exactly, and the float32
result equals the integer reference whatever the kernel's order is.  This is a condition on the inputs, not a
measurement of the code under test.

Why a 32-bit index cannot hide.  The float patterns are (k % 61) - 30 + (c % 7) and relatives: 61 and 13 are odd, so no
pattern repeats after 2^n rows.  An element index that wraps by 2^30 (a byte offset that wraps at 4 GiB), 2^31 or 2^32
elements therefore lands on other values; `assert_wrap_visible` evaluates the pattern at the wrapped index for the rows
around the boundaries and asserts that every such row differs from the true one.
"""
import numpy as np
import torch

E30, E31, E32 = 2 ** 30, 2 ** 31, 2 ** 32        # elements: a byte offset of 4 GiB, and the two 32-bit index limits
BOUNDARIES = (E30, E31, E32)
WINDOW = 64                                      # rows on each side of a boundary row, and at both ends of an array
CHUNK_ROWS = 2 ** 18                             # rows of 1024 floats: 1 GiB
EXACT = 2 ** 24                                  # integers of magnitude up to here are float32 values

VALUE_MAX = 36                                   # |value_pattern| <= 30 + 6
GRAD_MAX = 8                                     # |grad_pattern| <= 6 + 2
WEIGHT_MAX = 2                                   # weight_pattern is 0, 1 or 2


# ------------------------------------------------------------------------------------------------------------- windows
def windows(rows, C):
    """The row ranges [lo, hi) a test brings to the host: WINDOW rows at the start and at the end of a [rows, C] array,
    and WINDOW rows on each side of (and with) the rows that hold elements E30, E31 and E32 -- clipped to the array;
    a range that lies outside it is dropped."""
    out = []
    for lo, hi in [(0, WINDOW), (rows - WINDOW, rows)] + [(E // C - WINDOW, E // C + WINDOW + 1) for E in BOUNDARIES]:
        lo, hi = max(lo, 0), min(hi, rows)
        if hi > lo:
            out.append((lo, hi))
    return out


def window_rows(rows, C):
    """int64 numpy: the rows of windows(rows, C), ascending, each once."""
    w = windows(rows, C)
    return np.unique(np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in w])) if w else np.zeros(0, np.int64)


def chunks(rows, step=CHUNK_ROWS):
    """[k0, k1) ranges of at most `step` rows that cover [0, rows)."""
    return [(k0, min(k0 + step, rows)) for k0 in range(0, rows, step)]


# ------------------------------------------------------------------------------------------------------------ patterns
def _two_term(k, C, mod_k, shift_k, mod_c):
    cols = torch.arange(C, dtype=torch.int64, device=k.device)
    return ((k % mod_k - shift_k)[:, None] + (cols % mod_c)[None, :]).to(torch.float32)


def value_pattern(k, C):
    """float32 [n, C] for absolute rows k (int64 [n]): (k % 61) - 30 + (c % 7), integers in [-30, 36]."""
    return _two_term(k, C, 61, 30, 7)


def grad_pattern(k, C):
    """float32 [n, C]: (k % 13) - 6 + (c % 3), integers in [-6, 8]: an upstream gradient."""
    return _two_term(k, C, 13, 6, 3)


def small_pattern(k, C):
    """float32 [n, C]: (k % 5) - 2 + (c % 3), integers in [-2, 4]: features whose squared differences (at most 36) can be
    summed over a few hundred edges and 1024 columns below 2^24."""
    return _two_term(k, C, 5, 2, 3)


def moment1_pattern(k, C):
    """float32 [n, C]: grad_pattern(k + 5) / 8 -- a first moment of an optimizer state, of either sign."""
    return grad_pattern(k + 5, C) * 0.125


def moment2_pattern(k, C):
    """float32 [n, C]: value_pattern(k + 3)^2 / 2 -- a second moment, never negative."""
    v = value_pattern(k + 3, C)
    return v * v * 0.5


def table_pattern(r, C):
    """float32 [n, C]: r * C + c, the flat element index itself -- exact while rows * C <= 2^24."""
    cols = torch.arange(C, dtype=torch.int64, device=r.device)
    return (r[:, None] * C + cols[None, :]).to(torch.float32)


def mix(k):
    """A 31-bit hash of an index below 2^31.  Written so that no intermediate reaches 2^63: the same integers come out of
    torch int64 tensors, numpy int64 arrays and Python ints."""
    h = k * 0x9E3779B1
    h = ((h ^ (h >> 15)) & 0x7FFFFFFF) * 0x2C1B3C6D
    h = h ^ (h >> 12)
    return h & 0x7FFFFFFF


def weight_pattern(k):
    """float32 [n]: mix(k) % 3, a weight in {0, 1, 2} per sample."""
    return (mix(k) % 3).to(torch.float32)


def row_pattern(k, M, big=None):
    """int32 [n]: the feature row of sample k, hashed into [-1, M] -- both out-of-range values occur (one sample in 1024
    is outside, half of them at -1 and half at M).  The table is loaded unevenly on purpose, so that every kernel of
    reduce_rows runs: the rows of [0, M / 4) take 1000 samples in 1024 (about 4 T / M each: long rows, chunks and a join),
    the EVEN rows of [M / 4, M) take 23 in 1024 (about T / (33 M) each: short rows), the odd rows of [M / 4, M) are empty.
    big = (first sample, count, row): those samples name `row` instead -- the one row with 2^17 samples."""
    h = mix(k)
    u, v = h % 1024, h >> 10
    q = max(M // 4, 1)
    sparse = q + 2 * (v % max((M - q + 1) // 2, 1))
    outside = (v % 2) * (M + 1) - 1                                   # -1 or M
    r = _where(u < 1000, v % q, sparse)
    r = _where(u == 1023, outside, r)
    if big is not None:
        first, count, row = big
        r = _where((k >= first) & (k < first + count), row, r)
    return r.to(torch.int32) if isinstance(r, torch.Tensor) else r


def _where(cond, a, b):
    if isinstance(cond, torch.Tensor):
        return torch.where(cond, a if isinstance(a, torch.Tensor) else torch.full_like(b, a), b)
    if isinstance(cond, np.ndarray):
        return np.where(cond, a, b)
    return a if cond else b


def sparse_grad_rows(rows, C, every=4099):
    """int64 numpy: the rows a lazy optimizer test gives a gradient -- the window rows and every 4099th row (a prime: no
    power of two of rows apart)."""
    return np.unique(np.concatenate([window_rows(rows, C), np.arange(0, rows, every, dtype=np.int64)]))


# --------------------------------------------------------------------------------------------------- wrap must be seen
def wrapped_rows(pattern, k0, k1, C, shift):
    """What rows [k0, k1) of a [rows, C] array would hold if the flat element index e = k * C + c lost `shift`: the
    pattern at e - shift.  This is the 32-bit mutation of a reference (an index kept in 32 bits is e - 2^32, a byte
    offset kept in 32 bits e - 2^30, a sign-extended one e - 2^31 more)."""
    e0, e1 = k0 * C - shift, k1 * C - shift
    assert e0 >= 0, "the rows must lie behind the shift"
    r0, r1 = e0 // C, -(-e1 // C)
    flat = pattern(torch.arange(r0, r1, dtype=torch.int64), C).reshape(-1)
    return flat[e0 - r0 * C:e1 - r0 * C].reshape(k1 - k0, C)


def assert_wrap_visible(pattern, rows, C, shifts=BOUNDARIES):
    """Asserts that in every window row of a [rows, C] array that lies behind a shift, the pattern read at the wrapped
    index differs from the true row in at least one column -- so an equality over the row fails.  Returns the number of
    rows looked at (0 means the array crosses no boundary: the caller's shape is wrong)."""
    looked = 0
    for shift in shifts:
        first = -(-shift // C)                                        # the first row that lies wholly behind the shift
        for lo, hi in windows(rows, C):
            lo = max(lo, first)
            if hi <= lo:
                continue
            true = pattern(torch.arange(lo, hi, dtype=torch.int64), C)
            wrap = wrapped_rows(pattern, lo, hi, C, shift)
            same = ~(true != wrap).any(dim=1)
            assert not bool(same.any()), f"rows {(torch.nonzero(same)[:, 0] + lo).tolist()} look the same {shift} elements back"
            looked += hi - lo
    return looked


def assert_exact(terms, max_abs, what=""):
    """The condition that makes a float32 sum of `terms` integers of magnitude <= max_abs exact in any order."""
    worst = int(terms) * int(max_abs)
    assert worst < EXACT, f"{what}: worst partial sum {worst} is not below 2^24"
    return worst


# ------------------------------------------------------------------------------------------------------------ samples
PERIOD = 750                                     # samples, and rays, of one period of the ray pattern
PERIOD_STARTS = (0, 1, 64, 128, 193, 493)        # first samples of its rays: lengths 1, 63, 64, 65, 300 and 257
LONG_RAY = 2 ** 17


def big_row_of(M, long_ray=LONG_RAY):
    """(first sample, count, row) of the one feature row with `long_ray` samples: an odd row of [M / 4, M), which the hash
    leaves empty, named by the samples from 3 * 2^19 on."""
    return (3 * 2 ** 19, long_ray, M // 4 + 1)


def default_long_rays(T, C, long_ray=LONG_RAY):
    """(first sample, length) of the hand-placed rays: one of `long_ray` samples, and one of 200 samples around each of the
    samples whose rows hold elements E31 and E32 of a [T, C] array (where T reaches them)."""
    out = [(min(PERIOD * 1000, (T // (4 * PERIOD)) * PERIOD), long_ray)]
    for E in (E31, E32):
        s = E // C
        if 100 <= s < T:
            out.append((s - 100, 200))
    return out


def ray_cuts(T, long_rays):
    """int64 numpy, ascending, cuts[0] = 0: the first sample of every non-empty ray.  Ray q is non-empty iff q is a cut: it
    owns the samples from q to the next cut (T behind the last), so ray index and sample index run in step -- a [Q, C]
    array of per-ray values crosses the element boundaries where the [T, C] array of per-sample values does.  All other
    rays are empty.  The periodic rays have 1, 63, 64, 65, 300 and 257 samples; `long_rays` (first sample, length) replace
    what they cover."""
    base = (np.arange(0, T, PERIOD, dtype=np.int64)[:, None] + np.asarray(PERIOD_STARTS, np.int64)[None, :]).reshape(-1)
    cuts = base[base < T]
    for first, length in long_rays:
        a, b = int(first), min(int(first) + int(length), T)
        assert 0 <= a < b
        cuts = np.concatenate([cuts[(cuts <= a) | (cuts >= b)], np.asarray([a] + ([b] if b < T else []), np.int64)])
    return np.unique(cuts)


class Synthetic:
    """Hand-made sample lists of T samples over Q = T rays (see ray_cuts) whose rows are row_pattern's.
    .samples: the RaySamples; .cuts: ray_cuts; .ray_chunks: [k0, k1) ranges of at most `chunk` samples that end on ray
    ends -- samples k0 .. k1 - 1 are exactly the samples of rays k0 .. k1 - 1."""

    def __init__(self, T, Q, long_rays, M, big_row=None, device="cpu", chunk=CHUNK_ROWS // 2):
        from svox_t_amd.samples import RaySamples
        assert Q == T, "the ray pattern gives a ray index to every sample index"
        self.T, self.Q, self.M, self.big_row, self.device = T, Q, M, big_row, device
        self.cuts = ray_cuts(T, long_rays)
        ext = np.concatenate([self.cuts, [T]])
        self.longest_ray = int(np.diff(ext).max())
        cuts_d = torch.from_numpy(ext).to(device)
        idx = torch.arange(T + 1, dtype=torch.int64, device=device)
        offsets = cuts_d[torch.searchsorted(cuts_d, idx, right=False)]
        ray = cuts_d[torch.searchsorted(cuts_d, idx[:T], right=True) - 1].to(torch.int32)
        row = row_pattern(idx[:T], M, big_row)
        z = torch.zeros(T, dtype=torch.float32, device=device)
        self.samples = RaySamples(offsets, ray, row, z, z + 1)
        self.ray_chunks = []
        k0 = 0
        while k0 < T:
            k1 = int(ext[np.searchsorted(ext, k0 + chunk, side="right") - 1])
            assert k1 > k0, "a ray is longer than a chunk"
            self.ray_chunks.append((k0, k1))
            k0 = k1

    def segment(self, k0, k1):
        """(start, end) int64 [k1 - k0], LOCAL to the chunk: the first sample of sample k's ray and the one behind its last."""
        s = self.samples
        ray = s.ray[k0:k1].long()
        return ray - k0, s.offsets[ray + 1] - k0


def synthetic_samples(T, Q, long_rays, M=4096, big_row=None, device="cpu", chunk=CHUNK_ROWS // 2):
    """The hand-made RaySamples of a test (a Synthetic: .samples is the RaySamples).  Ray lengths 0, 1, 63, 64, 65, 257 and
    300, the rays of `long_rays` -- default_long_rays: one of 2^17 samples, one across the row of element E31, one across
    the row of element E32 --, hashed rows, and with big_row = (first sample, count, row) one row of 2^17 samples."""
    return Synthetic(T, Q, long_rays, M, big_row, device, chunk)


# ---------------------------------------------------------------------------------------------------------- references
def as_float32(ref):
    """An integer (or float64) reference as float32, after checking that it loses nothing."""
    assert ref.numel() == 0 or int(ref.abs().max()) < EXACT, "the reference leaves the exact range"
    return ref.to(torch.float32)


def ref_gather(table, row):
    """table[row], zeros where row is outside [0, M) -- no arithmetic: the table's own dtype and bits."""
    M = table.shape[0]
    row = row.long()
    inside = (row >= 0) & (row < M)
    out = table[row.clamp(0, max(M - 1, 0))]
    out[~inside] = 0
    return out


def ref_segment_sum(values, index, n, acc=None):
    """int64 [n, C]: acc[i] += the sum of values[k] over the k with index[k] == i (an index outside [0, n) takes no part).
    values hold integers.  Pass the returned tensor back in as `acc` to go on with the next chunk."""
    if acc is None:
        acc = torch.zeros((n, values.shape[1]), dtype=torch.int64, device=values.device)
    index = index.long()
    inside = (index >= 0) & (index < n)
    acc.index_add_(0, index[inside], values[inside].to(torch.int64))
    return acc


def ref_segment_count(index, n, acc=None):
    """int64 [n]: the number of k with index[k] == i, added to acc."""
    if acc is None:
        acc = torch.zeros((n,), dtype=torch.int64, device=index.device)
    index = index.long()
    inside = (index >= 0) & (index < n)
    acc.index_add_(0, index[inside], torch.ones_like(index[inside]))
    return acc


def ref_segment_max(values, index, n, acc=None):
    """float32 [n, C]: the running maximum per index, from -inf (a maximum is the same in every precision and order)."""
    if acc is None:
        acc = torch.full((n, values.shape[1]), float("-inf"), dtype=torch.float32, device=values.device)
    index = index.long()
    inside = (index >= 0) & (index < n)
    acc.index_reduce_(0, index[inside], values[inside], "amax", include_self=True)
    return acc


def ref_segment_cumsum(values, start, end, exclusive=False, reverse=False):
    """int32 [n, C]: the running sum of values (integers) within whole segments; sample k's segment is start[k] .. end[k] - 1
    (local indices, as Synthetic.segment gives them).  exclusive: without the sample itself; reverse: from the segment's
    last sample towards its first.  int32, not int64, halves the temporaries: the caller's bound (below 2^24 for the whole
    chunk) is far inside it."""
    v = values.to(torch.int32)
    P = v.cumsum(0, dtype=torch.int32)
    zero = torch.zeros_like(P[:1])
    before = torch.cat([zero, P])                                     # before[i] = the sum of v[0 .. i - 1]
    incl = P - before[start]
    if reverse:
        incl = (before[end] - before[start]) - incl + v
    return incl - v if exclusive else incl


def ref_accumulate(w, values, ray, n):
    """int64 [n, C]: out[q] = the sum over the samples of ray q of w * values.  Both hold small integers: the single
    product w * v (|w v| <= WEIGHT_MAX * VALUE_MAX) is formed in their own dtype, where it is exact; the sum is int64."""
    return ref_segment_sum(w[:, None] * values, ray, n)


def ref_accumulate_grads(w, values, ray, grad_out):
    """(grad_w float64 [n], grad_values [n, C]) for grad_out [Q, C]: grad_w[k] = sum_c g[ray[k], c] * values[k, c], summed in
    float64; grad_values[k, c] = w[k] * g[ray[k], c], ONE product of two small integers, exact in the inputs' dtype (no
    sum to widen).  A sample whose ray is outside [0, Q) gets zeros."""
    Q = grad_out.shape[0]
    ray = ray.long()
    inside = (ray >= 0) & (ray < Q)
    g = grad_out[ray.clamp(0, max(Q - 1, 0))] * inside[:, None].to(grad_out.dtype)
    return (g * values).sum(1, dtype=torch.float64), w[:, None] * g
