"""Restatement of the per-sample interface (include/svoxt.h, svoxt_ray_samples_* / svoxt_sample_weights_* /
svoxt_sample_accumulate_*) on the CPU.

TEST INFRASTRUCTURE ONLY.  The reference has no such operators.  The lists are tests.depth_restate.march's steps (the
oracle's stepping, float32 in the reference's operation order) concatenated and stable-sorted by ray; the two primitives
are tied to the C++ oracle and to depth_restate at the anchors of tests/test_samples_host.py.

    lists(tree, rays, opt, min_sigma=None)        Lists: offsets int64 [Q + 1], row / ray int32 [T], depth / length float32 [T]
    weights(length, sigma, offsets, dtype)        (w [T], alpha [Q]) torch; float32: the kernels' sequence, per ray in list order
                                                      sigma > 0:  att = expf(-(length * sigma));  w = T * (1 - att);  T *= att
                                                      else:       w = 0, T unchanged                  alpha = 1 - T_end
                                                  (expf: O.expf, the kernels' own); float64: the same in torch ops, autograd
                                                  through `sigma`
    accumulate(w, values, offsets, dtype)         [Q, C] ([Q] with values None): acc += w * v per ray in list order
    grad_sigma_scale(length, sigma, offsets, grad_w, grad_alpha)
                                                  [T] float64, the "tight" scale of grad_sigma: its addends priced one by
                                                  one, the suffix sum by the full sum it is subtracted down from, as
                                                  depth_restate.moments_grad_scale prices them:
                                                      length_k (|gw_k| T_{k+1} + sum_all_j |gw_j| w_j + |ga| T_end)

The float32 sequence of the kernels' backward (svoxt_sample_weights_bwd), two forward-running sweeps per ray over the
samples with sigma > 0, every product and sum rounded to float32, no contraction:
    sweep 1:  att = expf(-(length * sigma));  w = T * (1 - att);  T *= att;  total += gw * w           -> total, T_end
              tail = ga * T_end
    sweep 2:  (T = 1 again) att, w, T *= att as above;  total -= gw * w;
              grad_sigma = length * ((gw * T - total) + tail)                                          (T: after the sample)
and of accumulate's: grad_w = sum_c g[ray, c] * values[k, c] added in ascending c from 0; grad_values[k, c] = w[k] * g[ray, c].
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from oracle import oracle as O
from tests.depth_restate import march


class Lists(NamedTuple):
    offsets: np.ndarray
    row: np.ndarray
    ray: np.ndarray
    depth: np.ndarray
    length: np.ndarray


def lists(tree: O.Tree, rays, opt, min_sigma=None) -> Lists:
    m = march(tree, rays, opt)
    if m.steps:
        ids = torch.cat([s[0] for s in m.steps])
        t = torch.cat([s[1] for s in m.steps])
        delta_t = torch.cat([s[2] for s in m.steps])
        row = torch.cat([s[3] for s in m.steps])
    else:
        ids = row = torch.zeros(0, dtype=torch.int64)
        t = delta_t = torch.zeros(0, dtype=torch.float32)
    if min_sigma is not None:
        keep = torch.from_numpy(tree.features)[row, tree.K - 1] > np.float32(min_sigma)
        ids, t, delta_t, row = ids[keep], t[keep], delta_t[keep], row[keep]
    order = torch.sort(ids, stable=True).indices           # steps are in march order: a stable sort keeps it within a ray
    ids, t, delta_t, row = ids[order], t[order], delta_t[order], row[order]
    ds = m.delta_scale[ids]
    depth = ds * t                                          # float32, this operand order
    length = delta_t * ds
    offsets = np.zeros(m.Q + 1, dtype=np.int64)
    np.cumsum(np.bincount(ids.numpy(), minlength=m.Q), out=offsets[1:])
    return Lists(offsets, row.numpy().astype(np.int32), ids.numpy().astype(np.int32), depth.numpy(), length.numpy())


def _positions(offsets):
    """[(rays, samples)] for list position 0, 1, ...: the rays that have such a sample and its index."""
    offsets = torch.as_tensor(np.asarray(offsets), dtype=torch.int64)
    counts = offsets[1:] - offsets[:-1]
    out = []
    for j in range(int(counts.max()) if counts.numel() else 0):
        r = torch.nonzero(counts > j).squeeze(1)
        out.append((r, offsets[r] + j))
    return out


def weights(length, sigma, offsets, dtype=torch.float64):
    f32 = dtype == torch.float32
    assert f32 or dtype == torch.float64
    length32 = torch.as_tensor(np.asarray(length), dtype=torch.float32)
    sigma = torch.as_tensor(sigma)
    sigma32 = sigma.detach().to(torch.float32)
    Q, T = len(offsets) - 1, length32.shape[0]
    light = torch.ones(Q, dtype=dtype)
    w = torch.zeros(T, dtype=dtype)
    for r, k in _positions(offsets):
        pos = sigma32[k] > 0
        r, k = r[pos], k[pos]
        if f32:
            att = torch.from_numpy(O.expf((-(length32[k] * sigma32[k])).numpy()))
        else:
            att = torch.exp(-(length32[k].to(dtype) * sigma[k].to(dtype)))
        w = w.index_put((k,), light[r] * (1.0 - att))
        light = light.index_put((r,), light[r] * att)
    return w, 1.0 - light


def accumulate(w, values, offsets, dtype=torch.float64):
    w = torch.as_tensor(w).to(dtype)
    Q = len(offsets) - 1
    if values is None:
        out = torch.zeros(Q, dtype=dtype)
        for r, k in _positions(offsets):
            out = out.index_put((r,), out[r] + w[k])
        return out
    values = torch.as_tensor(values).to(dtype)
    out = torch.zeros((Q, values.shape[1]), dtype=dtype)
    for r, k in _positions(offsets):
        out = out.index_put((r,), out[r] + w[k, None] * values[k])
    return out


def grad_sigma_scale(length, sigma, offsets, grad_w, grad_alpha):
    length = np.asarray(length, dtype=np.float64)
    sigma64 = torch.as_tensor(np.asarray(sigma), dtype=torch.float64)
    gw = np.zeros(length.shape[0]) if grad_w is None else np.abs(np.asarray(grad_w, dtype=np.float64))
    Q = len(offsets) - 1
    ga = np.zeros(Q) if grad_alpha is None else np.abs(np.asarray(grad_alpha, dtype=np.float64))
    w, alpha = weights(length, sigma64, offsets, torch.float64)
    w, t_end = w.numpy(), 1.0 - alpha.numpy()
    counts = np.diff(np.asarray(offsets))
    ray = np.repeat(np.arange(Q), counts)
    total = np.zeros(Q)
    np.add.at(total, ray, gw * w)
    # T after the sample: T_before * att = T_before - w
    t_after = np.ones(length.shape[0])
    light = np.ones(Q)
    for r, k in _positions(offsets):
        r, k = r.numpy(), k.numpy()
        light[r] = light[r] - w[k]
        t_after[k] = light[r]
    scale = length * (gw * t_after + total[ray] + ga[ray] * t_end[ray])
    return np.where(np.asarray(sigma) > 0, scale, 0.0)
