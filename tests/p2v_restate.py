"""Restatements of the reference's p2v (svox_t/csrc/p2v_kernel.cu:104-214) for the voxelize tests: the (point, voxel)
pair set in numpy float32 with the reference's expressions in the reference's order, and the values / gradients over
that pair set in float64 torch (autograd on the CPU)."""
from __future__ import annotations

import numpy as np
import torch

f32 = np.float32


def voxel_size(volume_size, n):
    return np.asarray(volume_size, f32) / f32(n - 1)


def pairs(points, volume_corner, volume_size, n, conv_radius, budget=1 << 22):
    """(point index, x, y, z) of every pair the reference visits with r <= conv_radius, all in float32:
    window = clamp(floor / ceil(((p -/+ cr) - corner) / vs)), p_voxel = i * vs + corner,
    r = sqrt((dx*dx + dy*dy) + dz*dz).  Non-finite points have no pair."""
    pts = np.asarray(points, f32).reshape(-1, 3)
    c = np.asarray(volume_corner, f32)
    vs = voxel_size(volume_size, n)
    cr = f32(conv_radius)
    keep = np.nonzero(np.isfinite(pts).all(1))[0]
    p = pts[keep]
    with np.errstate(invalid="ignore", over="ignore"):
        lo = np.clip(np.floor(((p - cr) - c) / vs), 0, n - 1).astype(np.int64)
        hi = np.clip(np.ceil(((p + cr) - c) / vs), 0, n - 1).astype(np.int64)
    out = []
    if len(p) == 0:
        return np.zeros((0, 4), np.int64)
    wmax = (hi - lo + 1).max(0)
    offs = np.stack(np.meshgrid(*[np.arange(w) for w in wmax], indexing="ij"), -1).reshape(-1, 3)
    step = max(1, budget // len(offs))
    for s in range(0, len(p), step):
        v = lo[s:s + step, None, :] + offs[None]                        # [m, O, 3]
        inside = (v <= hi[s:s + step, None, :]).all(-1)
        pv = v.astype(f32) * vs + c
        d = p[s:s + step, None, :] - pv
        with np.errstate(over="ignore"):                               # far points: r = inf, no pair
            r = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        m, o = np.nonzero(inside & (r <= cr))
        out.append(np.concatenate([keep[s + m][:, None], v[m, o]], 1))
    return np.concatenate(out, 0)


def pair_counts(pr, P, n):
    """per voxel [n, n, n, 1] and per point [P] number of pairs"""
    vox = np.bincount((pr[:, 1] * n + pr[:, 2]) * n + pr[:, 3], minlength=n ** 3).reshape(n, n, n, 1)
    return vox, np.bincount(pr[:, 0], minlength=P)


def terms(points, features, pr, volume_corner, volume_size, n, kernel_radius):
    """float64 torch tensors: per pair contribution w * f[:, F-1] and the leaves (points, features) of autograd.
    p_voxel is the float32 value the reference computes (i * vs + corner); the rest is float64."""
    vs = voxel_size(volume_size, n)
    pv = torch.from_numpy((pr[:, 1:].astype(f32) * vs + np.asarray(volume_corner, f32)).astype(np.float64))
    pts = torch.from_numpy(np.asarray(points, np.float64)).requires_grad_(True)
    ft = torch.from_numpy(np.asarray(features, np.float64)).requires_grad_(True)
    idx = torch.from_numpy(pr[:, 0])
    d = pts[idx] - pv
    r2 = (d * d).sum(1)
    kr = float(kernel_radius)
    w = torch.exp(-r2 / (2.0 * kr * kr))
    return w * ft[idx, -1], pts, ft


def forward_backward(points, features, pr, volume_corner, volume_size, n, kernel_radius, grad_output):
    """float64 over the pair set pr: (volume, Σ|contribution| per voxel, points gradient, its Σ|term| per element,
    gradient of features[:, F-1], its Σ|term|).  The gradients come from autograd; the Σ|term| scales from the
    reference's per-pair terms (p2v_kernel.cu:196-210)."""
    contrib, pts, ft = terms(points, features, pr, volume_corner, volume_size, n, kernel_radius)
    flat = torch.from_numpy((pr[:, 1] * n + pr[:, 2]) * n + pr[:, 3])
    vol = torch.zeros(n ** 3, dtype=torch.float64).index_add(0, flat, contrib)
    go = torch.from_numpy(np.asarray(grad_output, np.float64).reshape(-1))
    (vol * go).sum().backward()
    with torch.no_grad():
        idx = torch.from_numpy(pr[:, 0])
        vs = voxel_size(volume_size, n)
        pv = torch.from_numpy((pr[:, 1:].astype(f32) * vs + np.asarray(volume_corner, f32)).astype(np.float64))
        d = pts[idx] - pv
        kk = float(kernel_radius) ** 2
        w = torch.exp(-(d * d).sum(1) / (2.0 * kk))
        g = go[flat]
        scale = torch.zeros(n ** 3, dtype=torch.float64).index_add(0, flat, contrib.abs())
        pabs = torch.zeros_like(pts).index_add(0, idx, (g * ft[idx, -1] * w / kk).abs()[:, None] * d.abs())
        fabs = torch.zeros(ft.shape[0], dtype=torch.float64).index_add(0, idx, (g * w).abs())
    return (vol.detach().reshape(n, n, n, 1).numpy(), scale.reshape(n, n, n, 1).numpy(), pts.grad.numpy(),
            pabs.numpy(), ft.grad[:, -1].numpy(), fabs.numpy())
