"""Restatement of the gradient in the view direction (include/svoxt.h, svoxt_view_basis_bwd /
svoxt_shade_samples_bwd_basis) on the CPU.

TEST INFRASTRUCTURE ONLY.  The reference has no such operators.  Two float32 sequences, operation for operation, and a
float64 yardstick for each with a bound that is derived here, addend by addend.

    view_backward32(opt, vdirs, extra, basis, grad_basis)       grad_viewdirs float32 [Q, 3]: the kernel's sequence; basis
                                                                 is the forward's own output (O.basis), read for SG
    basis64(opt, v, extra)                                       [Q, basis_dim] float64 torch: the expressions of the
                                                                 forward in double, from the float32 constants and lobes;
                                                                 differentiable in v
    view_grad64(opt, vdirs, extra, grad_basis)                   float64 [Q, 3]: autograd through basis64
    view_bound(opt, vdirs, extra, grad_basis)                    float64 [Q, 3], derived below
    view_tight(opt, vdirs, extra, abs_grad_basis)                float64 [Q, 3]: sum_i |g_i| A_i,a -- the gradient is linear
                                                                 in grad_basis, so an upstream error of that size moves it by
                                                                 at most this much
    basis_backward32(features, offsets, row, ray, opt, values, g_values, activate)     grad_basis float32 [Q, basis_dim]
    basis_grad64(...the same...)                                 float64 [Q, basis_dim]: the contraction in double from the
                                                                 same float32 inputs (values included: d is defined from
                                                                 the forward's own output, and the sum is linear in the
                                                                 rest, so there is nothing for autograd to add)
    basis_bound(...the same...)                                  float64 [Q, basis_dim]
    basis_tight(features, offsets, row, ray, opt, abs_t)         float64 [Q, basis_dim]: sum |t[k, c]| |f| for per-sample
                                                                 magnitudes abs_t [T, C] of the bracket grad_values * d

THE DEFINITIONS are the two sequences of include/svoxt.h; `_partials` below is the header's table of SH derivatives,
written once and evaluated twice: in float32 (the definition) and, with every difference turned into a sum of absolute
values, in float64 (A_i,a, the magnitude an addend's rounding errors are priced by).  u = 2^-24.

THE BOUND of view_backward32 against view_grad64, per ray and axis a.  The definition computes sum_i g_i P_i,a with P_i,a
an expression tree over x, y, z and float32 constants; the yardstick evaluates the same trees exactly (2^-53).  A tree
whose longest path holds d rounded operations returns sum_terms term (1 + theta), |theta| <= gamma_d, so its error is at
most gamma_d A_i,a, A the tree with |.| at every leaf and + for every -.  Then one rounding for g_i * P and one per add
into the accumulator, each add at most u of the running sum <= S_a = sum_i |g_i| A_i,a:
  SH    longest path 5 (component 12, Z: zz, 6 zz, - 3 xx, - 3 yy, C3[3] *; component 20 and 24 the same length), the
        product 1, n_a adds (n_a: the components with a partial on axis a):
            bound_a = (6 + n_a) u S_a
  SG    P_i,a = (b_i lobe[0]) lobe[1 + a]: 2 roundings, the product 1, n adds -- and b_i is the FORWARD's float32 output,
        not the exact exponential: its argument t = lobe[0] (dot - 1) is off by u (3 |lobe[0]| D + 2 |t|) (dot3: three
        roundings on D = sum_a |dir_a lobe[1 + a]|; the subtraction and the product one each, priced by |t| -- the
        subtraction's |dot - 1| |lobe[0]| = |t|), which is the relative error it gives e^t; pexpf adds 2 ulp = 4 u (its
        documented accuracy is ~1 ulp; priced at the 2 ulp the reference's expf is specified to) and the division by
        basis_dim u:
            bound_a = sum_i |g_i P_i,a| (3 + n + 5 + 3 |lobe[0]| D_i + 2 |t_i|) u
  ASG   P_i,a = (lobe[8 + a] E + (S E) (cx lobe[2 + a] + cy lobe[5 + a])) / bd: the longest path is dot3 (3), cx (1),
        cx lobe (1), the inner add (1), times SE (1), the outer add (1), the division (1): 9, the product with g 1, n adds.
        A_i,a = (|lobe[8 + a]| + D_S (2 lambda D_x |lobe[2 + a]| + 2 mu D_y |lobe[5 + a]|)) E / bd with D_S, D_x, D_y the
        dot products' sums of absolute values.  E is recomputed by the forward's sequence: its argument -lambda dot_x^2 -
        mu dot_y^2 is off by u (lambda (6 |dot_x| D_x + 3 dot_x^2) + mu (6 |dot_y| D_y + 3 dot_y^2)) (dot_x carries 3 u D_x,
        squared: 6 u |dot_x| D_x; two products and the subtraction: 3 u of each term), pexpf adds 4 u:
            bound_a = sum_i |g_i| A_i,a (10 + n + 4 + arg_i / u) u
All times 1.001 for the second-order terms (gamma_k <= 1.001 k u for k < 10^4).  An axis without addends has bound 0.

THE BOUND of basis_backward32 against basis_grad64, per ray and component: the addend (g d) f costs three roundings --
d = fl(sig (1 - sig)) from double, g * d, * f (two with activate = False: three is used for both) -- and each of the n = C
* (the ray's samples) adds at most u of the running sum <= S = sum |g d f|:
            bound = 1.001 (3 + n) u S
No exponential is involved.  A component outside [min_comp, max_comp] and a ray without samples have bound 0.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import oracle as O

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
SLACK = 1.001
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)
C4 = (2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431,
      -0.6690465435572892, 0.47308734787878004, -1.7701307697799304, 0.6258357354491761)


def _partials(x, y, z, bd, absolute=False):
    """{i: (X_i, Y_i, Z_i)} of the header's table (None: identically zero, not added), every operation in the dtype of
    x.  absolute: |x|, |y|, |z|, the constants' magnitudes and a sum for every difference -- A_i,a."""
    dt = x.dtype.type
    if absolute:
        x, y, z = np.abs(x), np.abs(y), np.abs(z)
        c = lambda v: dt(abs(f32(v)))                            # noqa: E731  (the float32 constant's value)
        k = lambda v: dt(abs(v))                                 # noqa: E731
        sub = lambda a, b: a + b                                 # noqa: E731
    else:
        c = lambda v: dt(f32(v))                                 # noqa: E731
        k = dt
        sub = lambda a, b: a - b                                 # noqa: E731
    xx, yy, zz = x * x, y * y, z * z
    xy, yz, xz = x * y, y * z, x * z
    P = {}
    if bd in (4, 9, 16, 25):
        P[1] = (None, c(-C1), None)
        P[2] = (None, None, c(C1))
        P[3] = (c(-C1), None, None)
    if bd in (9, 16, 25):
        P[4] = (c(C2[0]) * y, c(C2[0]) * x, None)
        P[5] = (None, c(C2[1]) * z, c(C2[1]) * y)
        P[6] = (c(C2[2]) * (k(-2) * x), c(C2[2]) * (k(-2) * y), c(C2[2]) * (k(4) * z))
        P[7] = (c(C2[3]) * z, None, c(C2[3]) * x)
        P[8] = (c(C2[4]) * (k(2) * x), c(C2[4]) * (k(-2) * y), None)
    a = sub(k(3) * xx, k(3) * yy)
    if bd in (16, 25):
        P[9] = (c(C3[0]) * (k(6) * xy), c(C3[0]) * a, None)
        P[10] = (c(C3[1]) * yz, c(C3[1]) * xz, c(C3[1]) * xy)
        P[11] = (c(C3[2]) * (k(-2) * xy), c(C3[2]) * sub(sub(k(4) * zz, xx), k(3) * yy), c(C3[2]) * (k(8) * yz))
        P[12] = (c(C3[3]) * (k(-6) * xz), c(C3[3]) * (k(-6) * yz), c(C3[3]) * sub(sub(k(6) * zz, k(3) * xx), k(3) * yy))
        P[13] = (c(C3[4]) * sub(sub(k(4) * zz, k(3) * xx), yy), c(C3[4]) * (k(-2) * xy), c(C3[4]) * (k(8) * xz))
        P[14] = (c(C3[5]) * (k(2) * xz), c(C3[5]) * (k(-2) * yz), c(C3[5]) * sub(xx, yy))
        P[15] = (c(C3[6]) * a, c(C3[6]) * (k(-6) * xy), None)
    if bd == 25:
        p, m = sub(k(3) * xx, yy), sub(xx, k(3) * yy)
        s1, s3, t3 = sub(k(7) * zz, k(1)), sub(k(7) * zz, k(3)), sub(k(21) * zz, k(3))
        P[16] = (c(C4[0]) * (y * p), c(C4[0]) * (x * m), None)
        P[17] = (c(C4[1]) * ((k(6) * xy) * z), c(C4[1]) * (z * a), c(C4[1]) * (y * p))
        P[18] = (c(C4[2]) * (y * s1), c(C4[2]) * (x * s1), c(C4[2]) * ((k(14) * xy) * z))
        P[19] = (None, c(C4[3]) * (z * s3), c(C4[3]) * (y * t3))
        P[20] = (None, None, c(C4[4]) * (z * sub(k(140) * zz, k(60))))
        P[21] = (c(C4[5]) * (z * s3), None, c(C4[5]) * (x * t3))
        P[22] = (c(C4[6]) * ((k(2) * x) * s1), c(C4[6]) * ((k(-2) * y) * s1), c(C4[6]) * (sub(xx, yy) * (k(14) * z)))
        P[23] = (c(C4[7]) * (z * a), c(C4[7]) * ((k(-6) * xy) * z), c(C4[7]) * (x * m))
        P[24] = (c(C4[8]) * (x * sub(k(4) * xx, k(12) * yy)), c(C4[8]) * (y * sub(k(4) * yy, k(12) * xx)), None)
    return P


def _xyz(vdirs, dt):
    v = np.ascontiguousarray(vdirs, dtype=f32).astype(dt)
    return v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy()


def _dot3(x, y, z, l):
    return x * l[0] + y * l[1] + z * l[2]


# ---------------------------------------------------------------------------------- view_basis: the definition, float32
def view_backward32(opt, vdirs, extra, basis, grad_basis):
    x, y, z = _xyz(vdirs, f32)
    Q, bd = x.shape[0], opt.basis_dim
    g = np.ascontiguousarray(grad_basis, dtype=f32)
    acc = [np.zeros(Q, f32) for _ in range(3)]
    with np.errstate(all="ignore"):
        if opt.format == O.FORMAT_SH:
            P = _partials(x, y, z, bd)
            for i in sorted(P):
                for a in range(3):
                    if P[i][a] is not None:
                        acc[a] = acc[a] + g[:, i] * P[i][a]
        elif opt.format == O.FORMAT_SG:
            b = np.ascontiguousarray(basis, dtype=f32)
            for i in range(bd):
                lobe = np.asarray(extra, dtype=f32)[i]
                s = b[:, i] * lobe[0]
                for a in range(3):
                    acc[a] = acc[a] + g[:, i] * (s * lobe[1 + a])
        elif opt.format == O.FORMAT_ASG:
            n = f32(bd)
            for i in range(bd):
                lobe = np.asarray(extra, dtype=f32)[i]
                S, dx, dy = _dot3(x, y, z, lobe[8:11]), _dot3(x, y, z, lobe[2:5]), _dot3(x, y, z, lobe[5:8])
                E = O.expf(-lobe[0] * dx * dx - lobe[1] * dy * dy)
                SE = S * E
                cx, cy = (f32(-2) * lobe[0]) * dx, (f32(-2) * lobe[1]) * dy
                for a in range(3):
                    acc[a] = acc[a] + g[:, i] * ((lobe[8 + a] * E + SE * (cx * lobe[2 + a] + cy * lobe[5 + a])) / n)
    return np.stack(acc, axis=1).astype(f32)


# ---------------------------------------------------------------------------------------- view_basis: the yardstick
def basis64(opt, v, extra=None):
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    bd = opt.basis_dim
    c = lambda t: float(f32(t))                                  # noqa: E731
    if opt.format == O.FORMAT_SH:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        out = [torch.full_like(x, c(0.28209479177387814))]
        if bd >= 4:
            out += [-c(C1) * y, c(C1) * z, -c(C1) * x]
        if bd >= 9:
            out += [c(C2[0]) * xy, c(C2[1]) * yz, c(C2[2]) * (2.0 * zz - xx - yy), c(C2[3]) * xz, c(C2[4]) * (xx - yy)]
        if bd >= 16:
            out += [c(C3[0]) * y * (3 * xx - yy), c(C3[1]) * xy * z, c(C3[2]) * y * (4 * zz - xx - yy),
                    c(C3[3]) * z * (2 * zz - 3 * xx - 3 * yy), c(C3[4]) * x * (4 * zz - xx - yy), c(C3[5]) * z * (xx - yy),
                    c(C3[6]) * x * (xx - 3 * yy)]
        if bd >= 25:
            out += [c(C4[0]) * xy * (xx - yy), c(C4[1]) * yz * (3 * xx - yy), c(C4[2]) * xy * (7 * zz - 1), c(C4[3]) * yz * (7 * zz - 3),
                    c(C4[4]) * (zz * (35 * zz - 30) + 3), c(C4[5]) * xz * (7 * zz - 3), c(C4[6]) * (xx - yy) * (7 * zz - 1),
                    c(C4[7]) * xz * (xx - 3 * yy), c(C4[8]) * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))]
        return torch.stack(out[:bd], dim=1)
    L = torch.from_numpy(np.asarray(extra, dtype=f32)).double()[:bd]
    if opt.format == O.FORMAT_SG:
        return torch.exp(L[:, 0] * (v @ L[:, 1:4].T - 1.0)) / bd
    S, dx, dy = v @ L[:, 8:11].T, v @ L[:, 2:5].T, v @ L[:, 5:8].T
    return S * torch.exp(-L[:, 0] * dx * dx - L[:, 1] * dy * dy) / bd


def view_grad64(opt, vdirs, extra, grad_basis):
    v = torch.from_numpy(np.ascontiguousarray(vdirs, dtype=f32)).double().requires_grad_(True)
    (basis64(opt, v, extra) * torch.from_numpy(np.asarray(grad_basis, dtype=f64))).sum().backward()
    return v.grad.numpy()


def _view_scales(opt, vdirs, extra, g):
    """(S float64 [Q, 3], W float64 [Q, 3]): S_a = sum_i |g_i| A_i,a and W_a = the same sum with every addend times its own
    operation count and forward error in units of u, the adds left out."""
    x, y, z = _xyz(vdirs, f64)
    Q, bd = x.shape[0], opt.basis_dim
    g = np.abs(np.asarray(g, dtype=f64))
    S, W = np.zeros((Q, 3)), np.zeros((Q, 3))
    if opt.format == O.FORMAT_SH:
        P = _partials(x, y, z, bd, absolute=True)
        for i in P:
            for a in range(3):
                if P[i][a] is not None:
                    S[:, a] += g[:, i] * P[i][a]
        return S, 6.0 * S
    L = np.asarray(extra, dtype=f32).astype(f64)[:bd]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    for i in range(bd):
        l = L[i]
        if opt.format == O.FORMAT_SG:
            D = ax * abs(l[1]) + ay * abs(l[2]) + az * abs(l[3])
            t = l[0] * (_dot3(x, y, z, l[1:4]) - 1.0)
            b = np.exp(t) / bd
            ops = 3.0 + 5.0 + 3.0 * abs(l[0]) * D + 2.0 * np.abs(t)
            for a in range(3):
                A = g[:, i] * b * abs(l[0]) * abs(l[1 + a])
                S[:, a] += A
                W[:, a] += A * ops
        else:
            DS = ax * abs(l[8]) + ay * abs(l[9]) + az * abs(l[10])
            Dx = ax * abs(l[2]) + ay * abs(l[3]) + az * abs(l[4])
            Dy = ax * abs(l[5]) + ay * abs(l[6]) + az * abs(l[7])
            dx, dy = _dot3(x, y, z, l[2:5]), _dot3(x, y, z, l[5:8])
            lam, mu = abs(l[0]), abs(l[1])
            E = np.exp(-l[0] * dx * dx - l[1] * dy * dy)
            arg = lam * (6.0 * np.abs(dx) * Dx + 3.0 * dx * dx) + mu * (6.0 * np.abs(dy) * Dy + 3.0 * dy * dy)
            ops = 10.0 + 4.0 + arg
            for a in range(3):
                A = g[:, i] * (abs(l[8 + a]) + DS * (2.0 * lam * Dx * abs(l[2 + a]) + 2.0 * mu * Dy * abs(l[5 + a]))) * E / bd
                S[:, a] += A
                W[:, a] += A * ops
    return S, W


def _adds(opt):
    """n_a: how many components hold a partial on axis a."""
    if opt.format != O.FORMAT_SH:
        return np.full(3, float(opt.basis_dim))
    one = np.ones(1, f64)
    P = _partials(one, one, one, opt.basis_dim, absolute=True)
    return np.array([sum(P[i][a] is not None for i in P) for a in range(3)], dtype=f64)


def view_tight(opt, vdirs, extra, abs_grad_basis):
    return _view_scales(opt, vdirs, extra, abs_grad_basis)[0]


def view_bound(opt, vdirs, extra, grad_basis):
    S, W = _view_scales(opt, vdirs, extra, grad_basis)
    return SLACK * U * (W + _adds(opt)[None, :] * S)


# ------------------------------------------------------------------------------ shade_samples in basis: the definition
def _segments(offsets, T):
    off = np.asarray(offsets).astype(np.int64)
    return np.maximum(off[:-1], 0), np.minimum(off[1:], T)


def _dims(opt, K):
    return (K - 1) // opt.basis_dim, opt.basis_dim


def basis_backward32(features, offsets, row, ray, opt, values, g_values=None, activate=True):
    feats = np.ascontiguousarray(features, dtype=f32)
    M, K = feats.shape
    C, bd = _dims(opt, K)
    row, ray = np.asarray(row).astype(np.int64), np.asarray(ray).astype(np.int64)
    T = row.shape[0]
    b, e = _segments(offsets, T)
    Q = b.shape[0]
    out = np.zeros((Q, bd), f32)
    if g_values is None or C == 0 or T == 0:
        return out
    g = np.ascontiguousarray(g_values, dtype=f32)
    sig = np.ascontiguousarray(values, dtype=f32)
    comps = np.arange(opt.min_comp, opt.max_comp + 1)
    n = np.maximum(e - b, 0)
    with np.errstate(all="ignore"):
        for j in range(int(n.max()) if Q else 0):
            q = np.flatnonzero(n > j)
            k = b[q] + j
            ok = (ray[k] == q) & (row[k] >= 0) & (row[k] < M)
            q, k = q[ok], k[ok]
            for c in range(C):
                t = g[k, c]
                if activate:
                    t = t * (sig[k, c].astype(f64) * (1.0 - sig[k, c].astype(f64))).astype(f32)
                out[q[:, None], comps[None, :]] = out[q[:, None], comps[None, :]] + t[:, None] * feats[row[k][:, None], c * bd + comps[None, :]]
    return out


def _contract64(features, offsets, row, ray, opt, t):
    """sum over a ray's segment of t[k, c] * features[row[k], c * bd + i] in float64, [Q, bd]; t float64 [T, C]."""
    feats = np.asarray(features, dtype=f32).astype(f64)
    M, K = feats.shape
    C, bd = _dims(opt, K)
    row, ray = np.asarray(row).astype(np.int64), np.asarray(ray).astype(np.int64)
    T = row.shape[0]
    b, e = _segments(offsets, T)
    Q = b.shape[0]
    out = np.zeros((Q, bd))
    if T == 0 or C == 0:
        return out
    n = np.maximum(e - b, 0)
    q_of = np.repeat(np.arange(Q), n)
    k = np.concatenate([np.arange(lo, hi) for lo, hi in zip(b, e)]) if n.sum() else np.zeros(0, np.int64)
    ok = (ray[k] == q_of) & (row[k] >= 0) & (row[k] < M)
    q_of, k = q_of[ok], k[ok]
    contrib = np.einsum("kc,kci->ki", t[k], feats[row[k], :C * bd].reshape(-1, C, bd))
    contrib[:, :opt.min_comp] = 0
    contrib[:, opt.max_comp + 1:] = 0
    np.add.at(out, q_of, contrib)
    return out


def _bracket64(values, g_values, activate):
    g = np.asarray(g_values, dtype=f32).astype(f64)
    if not activate:
        return g
    s = np.asarray(values, dtype=f32).astype(f64)
    return g * (s * (1.0 - s))


def basis_grad64(features, offsets, row, ray, opt, values, g_values=None, activate=True):
    if g_values is None:
        return np.zeros((len(offsets) - 1, opt.basis_dim))
    return _contract64(features, offsets, row, ray, opt, _bracket64(values, g_values, activate))


def basis_tight(features, offsets, row, ray, opt, abs_t):
    return _contract64(np.abs(np.asarray(features, dtype=f32)), offsets, row, ray, opt, np.abs(np.asarray(abs_t, dtype=f64)))


def basis_bound(features, offsets, row, ray, opt, values, g_values=None, activate=True):
    Q = len(offsets) - 1
    if g_values is None:
        return np.zeros((Q, opt.basis_dim))
    C, _ = _dims(opt, np.asarray(features).shape[1])
    b, e = _segments(offsets, np.asarray(row).shape[0])
    n = C * np.maximum(e - b, 0).astype(f64)
    S = basis_tight(features, offsets, row, ray, opt, _bracket64(values, g_values, activate))
    return SLACK * (3.0 + n)[:, None] * U * S


# --------------------------------------------------------------------------------- the forward's own error, for the chain
def sh_abs64(bd, vdirs):
    """[Q, bd] float64: the forward's SH expressions (basis_dim <= 9) with |.| at every leaf and + for every -: the forward's
    float32 value of component i lies within 3 u of this of the exact one (xx, the difference, the constant: three
    roundings on the longest path; component 6 is formed in double and rounded once)."""
    if bd > 9:
        raise NotImplementedError("sh_abs64: basis_dim <= 9")
    x, y, z = (np.abs(a) for a in _xyz(vdirs, f64))
    c = lambda t: abs(float(f32(t)))                             # noqa: E731
    out = [np.full_like(x, c(0.28209479177387814)), c(C1) * y, c(C1) * z, c(C1) * x, c(C2[0]) * x * y, c(C2[1]) * y * z,
           c(C2[2]) * (2.0 * z * z + x * x + y * y), c(C2[3]) * x * z, c(C2[4]) * (x * x + y * y)]
    return np.stack(out[:bd], axis=1)
