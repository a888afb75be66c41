"""Restatement of render_depth_moments (include/svoxt.h, svoxt_depth_moments_fwd / _bwd) as a CPU lock-step march in torch.

TEST INFRASTRUCTURE ONLY.  The reference has no such operator, so this file is what the HIP kernels are held to; it is
tied to the C++ oracle at three points (tests/test_depth_moments_host.py): its alpha column has the bits of
O.opacity_render, its m1 over an opaque volume the bits of O.render_depth, and its gradient for grad_output (0, 0, ga)
is O.volume_render_backward's with a one-column grad_output.

The stepping (ray set-up, leaf descent, step length) is oracle/torch_renderer.py's: float32 in the reference's operation
order, so the same leaves are visited.  Compositing runs in `dtype`: float32 reproduces the kernels' operation sequence
(exponential through O.expf, the kernels' own), float64 is the yardstick for tolerances and gradients.

    moments(tree, rays, opt, at, dtype)          [Q, 3] (m1, m2, alpha)
    moments_grad(tree, rays, opt, at, g)         [M, K] float64: autograd of sum(moments * g) at thresholds 0
    moments_grad_scale(tree, rays, opt, at, g)   [M, K] float64: sum_k delta_k (|c_k| T_{k+1} + sum_all_i w_i |c_i| + |ga| T_end),
                                                 the gradient's addends priced one by one, the suffix sum by the full
                                                 sequential sum it is subtracted down from (the "tight" scale of
                                                 O.volume_render_backward(..., want_abs="both"))
tree: O.Tree; rays: (origins, dirs, vdirs) numpy; opt: O.RenderOptions; at: "entry" | "mid"; g: [Q, 3] numpy.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import oracle as O
from oracle.torch_renderer import _dda_unit, _locate

_MARCHES: list = []      # (tree, origins, step_size, march): the march of a case is computed once


class _March:
    """Every leaf crossing with a feature row, step by step: steps[j] = (ray ids, t, delta_t, row), float32 / int64."""

    def __init__(self, tree: O.Tree, origins, dirs, step_size):
        f32 = torch.float32
        child = torch.from_numpy(tree.child.reshape(-1))
        data = torch.from_numpy(tree.data.reshape(-1))
        M, N = tree.M, tree.N
        offset = torch.from_numpy(tree.offset.astype(np.float32))
        scaling = torch.from_numpy(tree.scaling.astype(np.float32))
        o = torch.as_tensor(np.asarray(origins), dtype=f32)
        d = torch.as_tensor(np.asarray(dirs), dtype=f32)
        self.Q = o.shape[0]
        # per-ray set-up as oracle/torch_renderer.py:89-99 (float32, the reference's operation order)
        o = offset + scaling * o
        d = d * scaling
        nrm = torch.from_numpy(np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).numpy()))
        self.delta_scale = 1.0 / nrm
        d = d * self.delta_scale[:, None]
        inv = (1.0 / (d.double() + 1e-9)).float()
        tmin, tmax = _dda_unit(o, inv)
        self.hit = ~((tmax < 0) | (tmin > tmax))
        self.steps = []
        ids = torch.nonzero(self.hit).squeeze(1)
        t = tmin[ids].clone()
        while ids.numel():
            pos = o[ids] + t[:, None] * d[ids]
            slot, local, cube = _locate(child, N, pos)
            idx = data[slot].long()
            valid = (idx >= 0) & (idx < M)
            s_tmin, s_tmax = _dda_unit(local, inv[ids])
            delta_t = (s_tmax - s_tmin) / cube + np.float32(step_size)
            if valid.any():
                self.steps.append((ids[valid], t[valid], delta_t[valid], idx[valid]))
            t = t + delta_t
            keep = t < tmax[ids]
            ids, t = ids[keep], t[keep]


def march(tree: O.Tree, rays, opt) -> _March:
    for tr, org, ss, m in _MARCHES:
        if tr is tree and org is rays[0] and ss == float(opt.step_size):
            return m
    m = _March(tree, rays[0], rays[1], opt.step_size)
    _MARCHES.append((tree, rays[0], float(opt.step_size), m))
    del _MARCHES[:-8]
    return m


def _z32(m, ids, t, delta_t, at):
    ds = m.delta_scale[ids]
    if at == "entry":
        return ds * t
    assert at == "mid", at
    return ds * (t + np.float32(0.5) * delta_t)


def moments(tree: O.Tree, rays, opt, at="entry", dtype=torch.float64, features=None, early_stop=True):
    """[Q, 3] (m1, m2, alpha) in `dtype`, the semantics of svoxt_depth_moments_fwd: samples with sigma > opt.sigma_thresh
    (decided on the float32 table), until T <= opt.stop_thresh (early_stop False: the backward's convention, no stop).
    `features` (float64 torch, may require grad) replaces tree.features in the compositing."""
    m = march(tree, rays, opt)
    K = tree.K
    feats32 = torch.from_numpy(tree.features)
    f32 = dtype == torch.float32
    assert f32 or dtype == torch.float64
    feats = feats32.to(dtype) if features is None else features
    Q = m.Q
    m1 = torch.zeros(Q, dtype=dtype)
    m2 = torch.zeros(Q, dtype=dtype)
    light = torch.ones(Q, dtype=dtype)
    stopped = torch.zeros(Q, dtype=torch.bool)
    for ids, t, delta_t, row in m.steps:
        act = (feats32[row, K - 1] > opt.sigma_thresh) & ~stopped[ids]
        if not act.any():
            continue
        a, ta, da, ra = ids[act], t[act], delta_t[act], row[act]
        z32 = _z32(m, a, ta, da, at)
        if f32:
            # the kernels' sequence: att = pexpf(-delta_t * delta_scale * sigma); w = T * (1 - att); m1 += w * z;
            # m2 += w * (z * z); T *= att -- every product and sum rounded to float32
            x = ((-da) * m.delta_scale[a]) * feats32[ra, K - 1]
            att = torch.from_numpy(O.expf(x.numpy()))
            w = light[a] * (1.0 - att)
            z = z32
        else:
            att = torch.exp(-(da * m.delta_scale[a]).to(dtype) * feats[ra, K - 1])
            w = light[a] * (1.0 - att)
            z = z32.to(dtype)
        m1 = m1.index_put((a,), m1[a] + w * z)              # (a ray appears once in a step)
        m2 = m2.index_put((a,), m2[a] + w * (z * z))
        light = light.index_put((a,), light[a] * att)
        if early_stop:
            st = light[a].detach() <= opt.stop_thresh
            if st.any():
                s = a[st]
                scale = 1.0 / (1.0 - light[s].double())       # float(1.0 / (1.0 - double(T))), as the colour forward's
                m1 = m1.index_put((s,), m1[s] * scale.to(dtype))
                m2 = m2.index_put((s,), m2[s] * scale.to(dtype))
                stopped[s] = True
    return torch.stack([m1, m2, 1.0 - light], dim=1)


def _zero_thresholds(opt):
    o = O.RenderOptions.from_buffer_copy(opt)
    o.sigma_thresh, o.stop_thresh = 0.0, 0.0
    return o


def moments_grad(tree: O.Tree, rays, opt, at, grad_output):
    """[M, K] float64: d sum(moments * grad_output) / d features by autograd, at thresholds 0 without early stop."""
    feats = torch.from_numpy(tree.features).double().requires_grad_(True)
    out = moments(tree, rays, _zero_thresholds(opt), at, torch.float64, features=feats, early_stop=False)
    (out * torch.as_tensor(np.asarray(grad_output), dtype=torch.float64)).sum().backward()
    return feats.grad.numpy()


def moments_grad_scale(tree: O.Tree, rays, opt, at, grad_output):
    """[M, K] float64, non-zero in the sigma column only: sum over the samples of a row of
    delta_k (|c_k| T_{k+1} + sum_all_i w_i |c_i| + |ga| T_end), delta_k = delta_t delta_scale, c_k = g1 z_k + g2 z_k^2."""
    m = march(tree, rays, opt)
    K = tree.K
    feats32 = torch.from_numpy(tree.features)
    g = torch.as_tensor(np.asarray(grad_output), dtype=torch.float64)
    Q = m.Q
    light = torch.ones(Q, dtype=torch.float64)
    total = torch.zeros(Q, dtype=torch.float64)
    terms = []
    for ids, t, delta_t, row in m.steps:
        act = feats32[row, K - 1] > 0
        if not act.any():
            continue
        a, ta, da, ra = ids[act], t[act], delta_t[act], row[act]
        z = _z32(m, a, ta, da, at).double()
        delta = (da * m.delta_scale[a]).double()
        att = torch.exp(-delta * feats32[ra, K - 1].double())
        c = (g[a, 0] * z + g[a, 1] * (z * z)).abs()
        total[a] += light[a] * (1.0 - att) * c
        light[a] *= att
        terms.append((a, ra, delta, c * light[a]))
    scale = np.zeros((tree.M, K), dtype=np.float64)
    for a, ra, delta, ct in terms:
        np.add.at(scale[:, K - 1], ra.numpy(), (delta * (ct + total[a] + g[a, 2].abs() * light[a])).numpy())
    return scale
