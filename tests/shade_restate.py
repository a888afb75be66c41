"""Restatement of shade_samples (include/svoxt.h, svoxt_shade_samples_fwd / _bwd) in numpy on the CPU.

TEST INFRASTRUCTURE ONLY.  Every operation is a separate float32 operation in the header's sequence -- the
double-precision steps in float64, rounded where the kernel rounds -- from O.basis and O.expf; the gradient's sum per
table entry is tests.rows_restate's reduction of the per-sample contributions: samples in ascending index, chunks of 256
from 0, the partials in chunk order.  tests/test_shade_host.py anchors the contributions to a float64 autograd formula.

    basis(opt, vdirs, extra)                                  float32 [Q, basis_dim] ([Q, 0] for RGBA)
    forward(features, row, ray, opt, basis, activate)         (values float32 [T, C], sigma float32 [T])
    contributions(features, row, ray, opt, basis, values, g_values, g_sigma, activate)     float32 [T, K]
    grad(...the same...)                                      float32 [M, K]: the chunked sums
features float32 [M, K]; row, ray int [T]; opt: O.RenderOptions; values: forward's; g_values [T, C] / g_sigma [T] or None."""
import numpy as np

from oracle import oracle as O
from tests import rows_restate as R

f32, f64 = np.float32, np.float64


def dims(opt, K):
    """(C, basis_dim or 0 for RGBA)."""
    return O.out_data_dim(opt, K) - 1, (0 if opt.format == O.FORMAT_RGBA else opt.basis_dim)


def basis(opt, vdirs, extra=None):
    if opt.format == O.FORMAT_RGBA:
        return np.zeros((np.asarray(vdirs).shape[0], 0), f32)
    return O.basis(opt.format, opt.basis_dim, vdirs, extra)


def forward(features, row, ray, opt, basis, activate=True):
    feats = np.ascontiguousarray(features, f32)
    M, K = feats.shape
    C, bd = dims(opt, K)
    row, ray = np.asarray(row).astype(np.int64), np.asarray(ray).astype(np.int64)
    T = row.shape[0]
    inside = (row >= 0) & (row < M)
    r = np.where(inside, row, 0)
    values = np.zeros((T, C), f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(C):
            if bd:
                off = c * bd
                tmp = np.zeros(T, f32)
                for i in range(opt.min_comp, opt.max_comp + 1):
                    tmp = tmp + basis[ray, i] * feats[r, off + i]
            else:
                tmp = feats[r, c]
            values[:, c] = (1.0 / (1.0 + O.expf(-tmp).astype(f64))).astype(f32) if activate else tmp
    values[~inside] = 0
    sigma = np.where(inside, feats[r, K - 1], f32(0)).astype(f32) if M > 0 else np.zeros(T, f32)
    return values, sigma


def contributions(features, row, ray, opt, basis, values, g_values=None, g_sigma=None, activate=True):
    M, K = np.asarray(features).shape
    C, bd = dims(opt, K)
    ray = np.asarray(ray).astype(np.int64)
    T = ray.shape[0]
    v = np.zeros((T, K), f32)
    if g_sigma is not None:
        v[:, K - 1] = np.asarray(g_sigma, f32)
    if g_values is None:
        return v
    g = np.asarray(g_values, f32)
    sig = np.asarray(values, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(C):
            if not bd:
                v[:, c] = g[:, c] * (sig[:, c] * (f32(1) - sig[:, c])) if activate else g[:, c]
                continue
            d = (sig[:, c].astype(f64) * (1.0 - sig[:, c].astype(f64))).astype(f32)
            for i in range(opt.min_comp, opt.max_comp + 1):
                v[:, c * bd + i] = (g[:, c] * d) * basis[ray, i] if activate else g[:, c] * basis[ray, i]
    return v


def grad(features, row, ray, opt, basis, values, g_values=None, g_sigma=None, activate=True):
    M, K = np.asarray(features).shape
    v = contributions(features, row, ray, opt, basis, values, g_values, g_sigma, activate)
    return R.reduce(v, row, M, "sum", 0.0).reshape(M, K)
