"""Restatement of shade_samples with per-row rotations (include/svoxt.h, svoxt_shade_rot_*) on the CPU.

TEST INFRASTRUCTURE ONLY.  The reference has no such operator.  The float32 sequences of the header, operation for
operation, and one float64 yardstick with a bound for each of the three gradients that is derived here, addend by addend.

    rotate32(rotations, row, vdirs, ray)                  u float32 [T, 3]: rotated_dir's sequence per sample (rows and rays
                                                          outside their ranges are read at index 0; their samples are masked)
    forward32(features, row, ray, opt, rotations, vdirs, extra, activate)      (values [T, C], sigma [T]): O.basis on u
    features_grad32(...the same..., values, g_values, g_sigma)                 float32 [M, K]: rows_restate's fixed order
    gu32(features, row, ray, opt, rotations, vdirs, extra, values, g_values, activate)   float32 [T, 3]: gB, then
                                                          viewgrad_restate.view_backward32 at u with grad_basis = gB
    rotations_grad32(gu, row, ray, vdirs, shape)          float32 [M, d, d]: rows_restate's fixed order, nine columns a row
    viewdirs_grad32(gu, offsets, row, ray, rotations, Q)  float32 [Q, 3]: a ray's segment in list order
    grads64(...)                                          the yardstick: V.basis64 on R64[row] @ v64[ray], the contraction
                                                          and the sigmoid in double, autograd for all three gradients
    bounds(...)                                           (bound_features [M, K], bound_rotations [M, d, d], bound_viewdirs
                                                          [Q, 3]) float64, derived below

THE BOUNDS.  u = 2^-24; gamma_n <= 1.001 n u (n < 10^4) and 1.001 is also what absorbs every term of second order in u.
The yardstick differentiates the EXACT function of the float32 inputs, so every float32 intermediate's distance from its
exact value is priced, per sample k with row r, ray q, m = rotations[r], v = viewdirs[q] (hats are float32 values):
  (1) u^_a   three roundings on the longest path (product, add, add):        du_a = 3 u sum_b |m_ab v_b|
  (2) B^_i   the forward's rounding at u^ plus the move of u^:               dB_i = fwd_i + sum_a |dB_i/du_a| du_a
             fwd_i, SH: the longest path of any component holds 6 rounded operations (component 20: zz, 35 zz, - 30, zz *,
             + 3, C4[4] *; component 24 as long), priced at 7 u A_i, A_i the expression with |.| at every leaf and + for
             every - (sh_abs64); SG: B (3 |lobe[0]| D + 2 |t| + 5) u and ASG: (3 D_S E + |S| E (arg + 6)) u / basis_dim,
             viewgrad_restate's prices of the same expressions (argument, 4 u for expf, product / division).
             dB_i/du_a: autograd of V.basis64 at the exact u.
  (3) tmp^_c n = max_comp - min_comp + 1 products and n adds from 0:         dtmp_c = sum_i |F_ci| dB_i + (n + 1) u sum_i |B^_i F_ci|
  (4) sig^_c the sigmoid's slope is at most 1/4; expf is priced at 4 u of e, the rounded quotient and conversion at 2 u:
                                                                             dsig_c = dtmp_c / 4 + 6 u sig_c
  (5) d^_c   = fl(sig^ (1 - sig^)) through double, |1 - 2 sig| <= 1:         dd_c = dsig_c + u d_c
  (6) t^_c   = fl(g_c d^_c):                                                 dt_c = |g_c| dd_c + u |g_c d^_c|      (activate=False: 0)
A row's sum runs in chunks of 256 from 0 and then over the partials: an addend of a row of N samples passes through at most
n_r = min(N, 256) + ceil(N / 256) rounded adds, each at most u of the sum of the magnitudes.
features.grad, column (c, i): the addend fl(t^ B^) against t B, then the float32 sum of the row's addends:
      bound = 1.001 [ sum_k ( |t_c| dB_i + dt_c |B^_i| + u |t^_c B^_i| ) + n_r u sum_k |t^_c B^_i| ];  sigma column: n_r u sum |g_sigma|
  (7) gB^_i  C products and C adds from 0:                                   dgB_i = sum_c dt_c |F_ci| + (C + 1) u sum_c |t^_c F_ci|
  (8) gu^_a  the float32 sequence at (u^, gB^) against the exact derivative at (u^, gB^): viewgrad_restate.view_bound --
             for SG with B recomputed by the forward, whose error that bound prices --; linear in gB: view_tight(dgB);
             and the move of u^: |sum_b J_ab du_b| with J the Jacobian of u -> sum_i gB_i dB_i/du (autograd, double):
                                                                             dgu_a = view_bound_a + view_tight(dgB)_a + sum_b |J_ab| du_b
rotations.grad[r, a, b]: addend fl(gu^_a v_b), n_r addends:   1.001 [ sum_k (dgu_a |v_b| + u |gu^_a v_b|) + n_r u sum_k |gu^_a v_b| ]
viewdirs.grad[q, b]: addend fl(m_ab gu^_a), 3 n_q addends:    1.001 [ sum_k,a (|m_ab| dgu_a + u |m_ab gu^_a|) + 3 n_q u sum_k,a |m_ab gu^_a| ]
An entry without addends (a row never hit, a ray without samples, a column outside the component range or the 3 x 3
block) has bound 0: there the result must be exactly 0.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import oracle as O
from tests import rows_restate as R
from tests import viewgrad_restate as V

f32, f64 = np.float32, np.float64
U, SLACK = V.U, V.SLACK


def dims(opt, K):
    return (K - 1) // opt.basis_dim, opt.basis_dim


def _index(row, ray, M, Q):
    row, ray = np.asarray(row).astype(np.int64), np.asarray(ray).astype(np.int64)
    ok = (row >= 0) & (row < M) & (ray >= 0) & (ray < Q)
    return row, ray, ok, np.where((row >= 0) & (row < M), row, 0), np.where((ray >= 0) & (ray < Q), ray, 0)


def rotate32(rotations, row, vdirs, ray):
    m = np.ascontiguousarray(rotations, dtype=f32)[row][:, :3, :3]
    v = np.ascontiguousarray(vdirs, dtype=f32)[ray]
    with np.errstate(all="ignore"):
        return np.stack([m[:, a, 0] * v[:, 0] + m[:, a, 1] * v[:, 1] + m[:, a, 2] * v[:, 2] for a in range(3)], axis=1).astype(f32)


def sample_basis32(opt, rotations, row, vdirs, ray, extra):
    """(u [T, 3], B [T, basis_dim]) float32 for in-range rows and rays (index 0 stands in elsewhere)."""
    u = rotate32(rotations, row, vdirs, ray)
    with np.errstate(all="ignore"):
        return u, O.basis(opt.format, opt.basis_dim, u, extra)


def forward32(features, row, ray, opt, rotations, vdirs, extra=None, activate=True):
    feats = np.ascontiguousarray(features, f32)
    M, K = feats.shape
    Q = np.asarray(vdirs).shape[0]
    C, bd = dims(opt, K)
    row, ray, ok, r, q = _index(row, ray, M, Q)
    T = row.shape[0]
    _, B = sample_basis32(opt, rotations, r, vdirs, q, extra)
    values = np.zeros((T, C), f32)
    with np.errstate(all="ignore"):
        for c in range(C):
            tmp = np.zeros(T, f32)
            for i in range(opt.min_comp, opt.max_comp + 1):
                tmp = tmp + B[:, i] * feats[r, c * bd + i]
            values[:, c] = (1.0 / (1.0 + O.expf(-tmp).astype(f64))).astype(f32) if activate else tmp
    values[~ok] = 0
    inside = (row >= 0) & (row < M)
    sigma = np.where(inside, feats[r, K - 1], f32(0)).astype(f32)
    return values, sigma


def _bracket32(values, g_values, activate):
    g = np.ascontiguousarray(g_values, f32)
    if not activate:
        return g
    sig = np.ascontiguousarray(values, f32).astype(f64)
    with np.errstate(all="ignore"):
        return g * (sig * (1.0 - sig)).astype(f32)


def features_grad32(features, row, ray, opt, rotations, vdirs, extra, values, g_values=None, g_sigma=None, activate=True):
    M, K = np.asarray(features).shape
    Q = np.asarray(vdirs).shape[0]
    C, bd = dims(opt, K)
    row, ray, ok, r, q = _index(row, ray, M, Q)
    T = row.shape[0]
    con = np.zeros((T, K), f32)
    if g_sigma is not None:
        con[:, K - 1] = np.asarray(g_sigma, f32)
    if g_values is not None and C > 0:
        _, B = sample_basis32(opt, rotations, r, vdirs, q, extra)
        t = _bracket32(values, g_values, activate)
        with np.errstate(all="ignore"):
            for c in range(C):
                for i in range(opt.min_comp, opt.max_comp + 1):
                    con[:, c * bd + i] = np.where(ok, t[:, c] * B[:, i], f32(0))
    return R.reduce(con, row, M, "sum", 0.0).reshape(M, K)


def gu32(features, row, ray, opt, rotations, vdirs, extra, values, g_values=None, activate=True):
    feats = np.ascontiguousarray(features, f32)
    M, K = feats.shape
    Q = np.asarray(vdirs).shape[0]
    C, bd = dims(opt, K)
    row, ray, ok, r, q = _index(row, ray, M, Q)
    T = row.shape[0]
    if g_values is None or C == 0 or T == 0:
        return np.zeros((T, 3), f32)
    u, B = sample_basis32(opt, rotations, r, vdirs, q, extra)
    t = _bracket32(values, g_values, activate)
    gB = np.zeros((T, bd), f32)
    with np.errstate(all="ignore"):
        for c in range(C):
            for i in range(opt.min_comp, opt.max_comp + 1):
                gB[:, i] = gB[:, i] + t[:, c] * feats[r, c * bd + i]
        gu = V.view_backward32(opt, u, extra, B, gB)
    gu[~ok] = 0
    return gu


def rotations_grad32(gu, row, ray, vdirs, shape):
    M, d, _ = shape
    v = np.ascontiguousarray(vdirs, f32)
    row, ray, ok, r, q = _index(row, ray, M, v.shape[0])
    con = np.zeros((row.shape[0], d * d), f32)
    with np.errstate(all="ignore"):
        for a in range(3):
            for b in range(3):
                con[:, a * d + b] = np.where((ray >= 0) & (ray < v.shape[0]), gu[:, a] * v[q, b], f32(0))
    return R.reduce(con, row, M, "sum", 0.0).reshape(M, d, d)


def viewdirs_grad32(gu, offsets, row, ray, rotations, Q):
    rot = np.ascontiguousarray(rotations, f32)
    M = rot.shape[0]
    row, ray = np.asarray(row).astype(np.int64), np.asarray(ray).astype(np.int64)
    T = row.shape[0]
    lo, hi = V._segments(offsets, T)
    n = np.maximum(hi - lo, 0)
    out = np.zeros((Q, 3), f32)
    with np.errstate(all="ignore"):
        for j in range(int(n.max()) if Q else 0):
            qs = np.flatnonzero(n > j)
            k = lo[qs] + j
            keep = (ray[k] == qs) & (row[k] >= 0) & (row[k] < M)
            qs, k = qs[keep], k[keep]
            m = rot[row[k]]
            for a in range(3):
                for b in range(3):
                    out[qs, b] = out[qs, b] + m[:, a, b] * gu[k, a]
    return out


# -------------------------------------------------------------------------------------------------------- the yardstick
def _tensors64(features, rotations, vdirs, grad):
    mk = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).double().requires_grad_(grad)      # noqa: E731
    return mk(features), mk(rotations), mk(vdirs)


def _forward64(F, Rm, v, row, ray, opt, extra, activate):
    """values float64 [n, C] torch for the valid samples given by row / ray (int64 tensors)."""
    K = F.shape[1]
    C, bd = dims(opt, K)
    u = torch.einsum("kab,kb->ka", Rm[row][:, :3, :3], v[ray])
    B = V.basis64(opt, u, extra)
    lo, hi = opt.min_comp, opt.max_comp + 1
    coef = F[row][:, :C * bd].reshape(-1, C, bd)[:, :, lo:hi]
    tmp = (coef * B[:, None, lo:hi]).sum(-1)
    return torch.sigmoid(tmp) if activate else tmp


def grads64(features, row, ray, opt, rotations, vdirs, extra, g_values=None, g_sigma=None, activate=True):
    """(features.grad [M, K], rotations.grad [M, d, d], viewdirs.grad [Q, 3]) float64 by autograd."""
    F, Rm, v = _tensors64(features, rotations, vdirs, True)
    M, Q = F.shape[0], v.shape[0]
    row, ray, ok, _, _ = _index(row, ray, M, Q)
    loss = F.sum() * 0.0 + Rm.sum() * 0.0 + v.sum() * 0.0
    if g_values is not None:
        k = np.flatnonzero(ok)
        vals = _forward64(F, Rm, v, torch.from_numpy(row[k]), torch.from_numpy(ray[k]), opt, extra, activate)
        loss = loss + (vals * torch.from_numpy(np.asarray(g_values, f32)[k].astype(f64))).sum()
    if g_sigma is not None:
        k = np.flatnonzero((row >= 0) & (row < M))
        loss = loss + (F[torch.from_numpy(row[k]), -1] * torch.from_numpy(np.asarray(g_sigma, f32)[k].astype(f64))).sum()
    loss.backward()
    return F.grad.numpy(), Rm.grad.numpy(), v.grad.numpy()


def sh_abs64(bd, u):
    """[n, bd] float64: the forward's SH expressions with |.| at every leaf and + for every -."""
    x, y, z = np.abs(u[:, 0]), np.abs(u[:, 1]), np.abs(u[:, 2])
    c = lambda t: abs(float(f32(t)))                             # noqa: E731
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    C1, C2, C3, C4 = V.C1, V.C2, V.C3, V.C4
    out = [np.full_like(x, c(0.28209479177387814)), c(C1) * y, c(C1) * z, c(C1) * x,
           c(C2[0]) * xy, c(C2[1]) * yz, c(C2[2]) * (2.0 * zz + xx + yy), c(C2[3]) * xz, c(C2[4]) * (xx + yy),
           c(C3[0]) * y * (3 * xx + yy), c(C3[1]) * xy * z, c(C3[2]) * y * (4 * zz + xx + yy), c(C3[3]) * z * (2 * zz + 3 * xx + 3 * yy),
           c(C3[4]) * x * (4 * zz + xx + yy), c(C3[5]) * z * (xx + yy), c(C3[6]) * x * (xx + 3 * yy),
           c(C4[0]) * xy * (xx + yy), c(C4[1]) * yz * (3 * xx + yy), c(C4[2]) * xy * (7 * zz + 1), c(C4[3]) * yz * (7 * zz + 3),
           c(C4[4]) * (zz * (35 * zz + 30) + 3), c(C4[5]) * xz * (7 * zz + 3), c(C4[6]) * (xx + yy) * (7 * zz + 1),
           c(C4[7]) * xz * (xx + 3 * yy), c(C4[8]) * (xx * (xx + 3 * yy) + yy * (3 * xx + yy))]
    return np.stack(out[:bd], axis=1)


def _forward_basis_error(opt, u, extra, B):
    """fwd_i of (2): [n, bd] float64, in absolute terms (u included)."""
    bd = opt.basis_dim
    if opt.format == O.FORMAT_SH:
        return SLACK * 7.0 * U * sh_abs64(bd, u)
    L = np.asarray(extra, dtype=f32).astype(f64)[:bd]
    a = np.abs(u)
    out = np.zeros((u.shape[0], bd))
    for i in range(bd):
        l = L[i]
        if opt.format == O.FORMAT_SG:
            D = a @ np.abs(l[1:4])
            t = l[0] * (u @ l[1:4] - 1.0)
            out[:, i] = np.abs(B[:, i]) * (3.0 * abs(l[0]) * D + 2.0 * np.abs(t) + 5.0)
        else:
            DS, Dx, Dy = a @ np.abs(l[8:11]), a @ np.abs(l[2:5]), a @ np.abs(l[5:8])
            S, dx, dy = u @ l[8:11], u @ l[2:5], u @ l[5:8]
            E = np.exp(-l[0] * dx * dx - l[1] * dy * dy)
            arg = abs(l[0]) * (6.0 * np.abs(dx) * Dx + 3.0 * dx * dx) + abs(l[1]) * (6.0 * np.abs(dy) * Dy + 3.0 * dy * dy)
            out[:, i] = (3.0 * DS * E + np.abs(S) * E * (arg + 6.0)) / bd
    return SLACK * U * out


def _scatter(index, n, values):
    out = np.zeros((n,) + values.shape[1:])
    np.add.at(out, index, values)
    return out


def bounds(features, offsets, row, ray, opt, rotations, vdirs, extra, values, g_values=None, g_sigma=None, activate=True):
    """(bound_features [M, K], bound_rotations [M, d, d], bound_viewdirs [Q, 3]) float64: the docstring's derivation."""
    feats = np.ascontiguousarray(features, f32)
    rot = np.ascontiguousarray(rotations, f32)
    vd = np.ascontiguousarray(vdirs, f32)
    (M, K), d, Q = feats.shape, rot.shape[1], vd.shape[0]
    C, bd = dims(opt, K)
    row, ray, ok, _, _ = _index(row, ray, M, Q)
    bf, br, bv = np.zeros((M, K)), np.zeros((M, d, d)), np.zeros((Q, 3))
    inside = (row >= 0) & (row < M)
    n_row = _scatter(row[inside], M, np.ones(int(inside.sum())))
    n_row = np.minimum(n_row, R.CHUNK) + np.ceil(n_row / R.CHUNK)                   # the adds an addend passes through, at most
    if g_sigma is not None:
        bf[:, K - 1] = SLACK * n_row * U * _scatter(row[inside], M, np.abs(np.asarray(g_sigma, f32)[inside].astype(f64)))
    k = np.flatnonzero(ok)
    if g_values is None or C == 0 or k.size == 0:
        return bf, br, bv
    r, q = row[k], ray[k]
    m64, v64 = rot[r][:, :3, :3].astype(f64), vd[q].astype(f64)
    g = np.asarray(g_values, f32)[k].astype(f64)
    comps = np.arange(opt.min_comp, opt.max_comp + 1)
    n = comps.shape[0]
    Fk = feats[r][:, :C * bd].reshape(-1, C, bd).astype(f64)                        # [n, C, bd]
    absF = np.abs(Fk)
    # (1), (2)
    du = SLACK * 3.0 * U * np.einsum("kab,kb->ka", np.abs(m64), np.abs(v64))
    u_t = torch.from_numpy(np.einsum("kab,kb->ka", m64, v64)).requires_grad_(True)
    B_t = V.basis64(opt, u_t, extra)
    jac = np.zeros((k.size, bd, 3))                                                 # (SH1: a constant, no derivative)
    if B_t.requires_grad:
        jac = np.stack([torch.autograd.grad(B_t[:, i].sum(), u_t, retain_graph=True)[0].numpy() for i in range(bd)], axis=1)
    u32, B32 = sample_basis32(opt, rot, r, vd, q, extra)
    B32 = B32.astype(f64)
    dB = _forward_basis_error(opt, u32.astype(f64), extra, B32) + np.einsum("kia,ka->ki", np.abs(jac), du)
    # (3) .. (6)
    mask = np.zeros(bd)
    mask[comps] = 1.0
    dtmp = np.einsum("kci,ki->kc", absF, dB * mask) + SLACK * (n + 1) * U * np.einsum("kci,ki->kc", absF, np.abs(B32) * mask)
    if activate:
        tmp = np.einsum("kci,ki->kc", Fk, B_t.detach().numpy() * mask)
        sig = 1.0 / (1.0 + np.exp(-tmp))
        dex = sig * (1.0 - sig)
        dsig = 0.25 * dtmp + 6.0 * U * sig
        dd = dsig + U * dex
        s32 = np.asarray(values, f32)[k].astype(f64)
        d32 = (s32 * (1.0 - s32)).astype(f32).astype(f64)
        t_ex, t32 = g * dex, (g.astype(f32) * d32.astype(f32)).astype(f64)
        dt = SLACK * (np.abs(g) * dd + U * np.abs(g * d32))
    else:
        t_ex = t32 = g
        dt = np.zeros_like(g)
    # features.grad
    add = np.abs(t32)[:, :, None] * np.abs(B32)[:, None, :]                         # |t^ B^| [n, C, bd]
    err = np.abs(t_ex)[:, :, None] * dB[:, None, :] + dt[:, :, None] * np.abs(B32)[:, None, :] + U * add
    tot = _scatter(r, M, (err * mask).reshape(-1, C * bd)) + n_row[:, None] * U * _scatter(r, M, (add * mask).reshape(-1, C * bd))
    bf[:, :C * bd] = SLACK * tot
    # (7), (8)
    gB32 = np.einsum("kc,kci->ki", t32, Fk) * mask
    dgB = (np.einsum("kc,kci->ki", dt, absF) + SLACK * (C + 1) * U * np.einsum("kc,kci->ki", np.abs(t32), absF)) * mask
    gB_t = torch.from_numpy(np.einsum("kc,kci->ki", t_ex, Fk) * mask)
    J = np.zeros((k.size, 3, 3))
    gu_t = torch.autograd.grad((B_t * gB_t).sum(), u_t, create_graph=True)[0] if B_t.requires_grad else u_t.detach()
    if gu_t.requires_grad:
        for a in range(3):
            J[:, a, :] = torch.autograd.grad(gu_t[:, a].sum(), u_t, retain_graph=True)[0].numpy()
    dgu = V.view_bound(opt, u32, extra, gB32) + V.view_tight(opt, u32, extra, dgB) + np.einsum("kab,kb->ka", np.abs(J), du)
    with np.errstate(all="ignore"):
        gu = np.abs(V.view_backward32(opt, u32, extra, B32.astype(f32), gB32.astype(f32)).astype(f64))
    gu = gu + dgu                                                                  # (|gu^| from the restated sequence's own inputs, priced up)
    # rotations.grad
    av = np.abs(v64)
    e_r = dgu[:, :, None] * av[:, None, :] + U * gu[:, :, None] * av[:, None, :]
    s_r = gu[:, :, None] * av[:, None, :]
    br[:, :3, :3] = SLACK * (_scatter(r, M, e_r) + n_row[:, None, None] * U * _scatter(r, M, s_r))
    # viewdirs.grad: only the samples standing in their own ray's segment
    lo, hi = V._segments(offsets, row.shape[0])
    own = (k >= lo[q]) & (k < hi[q])
    am = np.abs(m64)
    e_v = np.einsum("kab,ka->kb", am, dgu) + U * np.einsum("kab,ka->kb", am, gu)
    s_v = np.einsum("kab,ka->kb", am, gu)
    n_q = _scatter(q[own], Q, np.ones(int(own.sum())))
    bv[:] = SLACK * (_scatter(q[own], Q, e_v[own]) + 3.0 * n_q[:, None] * U * _scatter(q[own], Q, s_v[own]))
    return bf, br, bv
