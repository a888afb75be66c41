"""Restatement of render_distortion (include/svoxt.h, svoxt_distortion_fwd / _bwd) as a CPU lock-step march in torch.

TEST INFRASTRUCTURE ONLY.  The reference has no such operator, so this file is what the HIP kernels are held to; it is
tied to the C++ oracle at two points (tests/test_distortion_host.py) -- its alpha column has the bits of
O.opacity_render, and its gradient for grad_output (0, ga) is O.volume_render_backward's with a one-column grad_output
-- and to the loss's definition, the O(n^2) sum over pairs, at a third.

The march is tests/depth_restate.py's (the oracle's stepping in float32: the same leaves are visited).  Compositing runs
in `dtype`: float32 reproduces the kernels' operation sequence, float64 is the yardstick for tolerances and gradients.

    distortion(tree, rays, opt, dtype)          [Q, 2] (L, alpha)
    distortion_grad(tree, rays, opt, g)         [M, K] float64: autograd of sum(distortion * g) at thresholds 0
    distortion_grad_scale(tree, rays, opt, g)   [M, K] float64: sum_k d_k (|gd| (|u_k| T_{k+1} + 2 L) + |ga| T_end), the
                                                gradient's addends priced one by one, the suffix sum by the full sum 2 L
                                                it is subtracted down from
    ray_samples(tree, rays, opt)                per ray: float64 arrays (w, s, d) of the samples with sigma > 0
tree: O.Tree; rays: (origins, dirs, vdirs) numpy; opt: O.RenderOptions; g: [Q, 2] numpy.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import oracle as O
from tests.depth_restate import _zero_thresholds, march


def distortion(tree: O.Tree, rays, opt, dtype=torch.float64, features=None, early_stop=True, shift=0.0):
    """[Q, 2] (L, alpha) in `dtype`, the semantics of svoxt_distortion_fwd: samples with sigma > opt.sigma_thresh (decided
    on the float32 table), until T <= opt.stop_thresh (early_stop False: the backward's convention, no stop).  `features`
    (float64 torch, may require grad) replaces tree.features in the compositing; `shift` is added to every s."""
    m = march(tree, rays, opt)
    K = tree.K
    feats32 = torch.from_numpy(tree.features)
    f32 = dtype == torch.float32
    assert f32 or dtype == torch.float64
    feats = feats32.to(dtype) if features is None else features
    Q = m.Q
    zeros = lambda: torch.zeros(Q, dtype=dtype)                     # noqa: E731
    A, D, Lb, Lu, sp = zeros(), zeros(), zeros(), zeros(), zeros()
    light = torch.ones(Q, dtype=dtype)
    stopped = torch.zeros(Q, dtype=torch.bool)
    seen = torch.zeros(Q, dtype=torch.bool)
    half = np.float32(0.5)
    for ids, t, delta_t, row in m.steps:
        act = (feats32[row, K - 1] > opt.sigma_thresh) & ~stopped[ids]
        if not act.any():
            continue
        a, ta, da, ra = ids[act], t[act], delta_t[act], row[act]
        ds32 = m.delta_scale[a]
        s32 = ds32 * (ta + half * da)
        d32 = da * ds32
        if f32:
            # the kernels' sequence, every product and sum rounded to float32
            att = torch.from_numpy(O.expf((((-da) * ds32) * feats32[ra, K - 1]).numpy()))
            s, d = s32, d32
        else:
            att = torch.exp(-d32.to(dtype) * feats[ra, K - 1])
            s, d = s32.to(dtype) + shift, d32.to(dtype)
        w = light[a] * (1.0 - att)
        Da = torch.where(seen[a], D[a] + A[a] * (s - sp[a]), D[a])   # (a ray appears once in a step)
        D = D.index_put((a,), Da)
        sp = sp.index_put((a,), s)
        seen[a] = True
        Lb = Lb.index_put((a,), Lb[a] + w * Da)
        Lu = Lu.index_put((a,), Lu[a] + (w * w) * d)
        A = A.index_put((a,), A[a] + w)
        light = light.index_put((a,), light[a] * att)
        if early_stop:
            st = light[a].detach() <= opt.stop_thresh
            if st.any():
                k = a[st]
                scale = (1.0 / (1.0 - light[k].double())).to(dtype)  # float(1.0 / (1.0 - double(T))), once per factor of w
                Lb = Lb.index_put((k,), (Lb[k] * scale) * scale)
                Lu = Lu.index_put((k,), (Lu[k] * scale) * scale)
                stopped[k] = True
    third = torch.tensor(1.0, dtype=dtype) / torch.tensor(3.0, dtype=dtype)
    return torch.stack([2.0 * Lb + Lu * third, 1.0 - light], dim=1)


def distortion_grad(tree: O.Tree, rays, opt, grad_output):
    """[M, K] float64: d sum(distortion * grad_output) / d features by autograd, at thresholds 0 without early stop."""
    feats = torch.from_numpy(tree.features).double().requires_grad_(True)
    out = distortion(tree, rays, _zero_thresholds(opt), torch.float64, features=feats, early_stop=False)
    (out * torch.as_tensor(np.asarray(grad_output), dtype=torch.float64)).sum().backward()
    return feats.grad.numpy()


def _sweep(tree: O.Tree, rays, opt):
    """The samples with sigma > 0 step by step in float64: [(ray ids, rows, w, s, d, D_k, T_{k+1})], and per ray L, T_end."""
    m = march(tree, rays, opt)
    K = tree.K
    feats32 = torch.from_numpy(tree.features)
    Q = m.Q
    f64 = torch.float64
    A, D, sp, L = (torch.zeros(Q, dtype=f64) for _ in range(4))
    light = torch.ones(Q, dtype=f64)
    recs = []
    for ids, t, delta_t, row in m.steps:
        act = feats32[row, K - 1] > 0
        if not act.any():
            continue
        a, ta, da, ra = ids[act], t[act], delta_t[act], row[act]
        ds32 = m.delta_scale[a]
        s = (ds32 * (ta + np.float32(0.5) * da)).double()
        d = (da * ds32).double()
        att = torch.exp(-d * feats32[ra, K - 1].double())
        w = light[a] * (1.0 - att)
        D[a] += A[a] * (s - sp[a])                                   # (the first sample: A == 0)
        sp[a] = s
        L[a] += 2.0 * w * D[a] + w * w * d / 3.0
        A[a] += w
        light[a] *= att
        recs.append((a, ra, w, s, d, D[a].clone(), light[a].clone()))
    return m, recs, L, light


def distortion_grad_scale(tree: O.Tree, rays, opt, grad_output):
    """[M, K] float64, non-zero in the sigma column only: sum over the samples of a row of
    d_k (|gd| (|u_k| T_{k+1} + 2 L) + |ga| T_end), u_k = 2 (D_k + E_k) + (2/3) w_k d_k."""
    m, recs, L, t_end = _sweep(tree, rays, opt)
    g = torch.as_tensor(np.asarray(grad_output), dtype=torch.float64).abs()
    Q = m.Q
    after = torch.zeros(Q, dtype=torch.float64)                      # sum_{j>k} w_j
    E = torch.zeros(Q, dtype=torch.float64)                          # sum_{j>k} w_j (s_j - s_k)
    sn = torch.zeros(Q, dtype=torch.float64)                         # s_{k+1}
    scale = np.zeros((tree.M, tree.K), dtype=np.float64)
    for a, ra, w, s, d, Dk, tn in reversed(recs):
        E[a] += after[a] * (sn[a] - s)                               # (the last sample: after == 0)
        u = 2.0 * (Dk + E[a]) + (2.0 / 3.0) * w * d
        np.add.at(scale[:, tree.K - 1], ra.numpy(),
                  (d * (g[a, 0] * (u.abs() * tn + 2.0 * L[a]) + g[a, 1] * t_end[a])).numpy())
        after[a] += w
        sn[a] = s
    return scale


def ray_samples(tree: O.Tree, rays, opt):
    """Per ray, in march order: float64 numpy arrays (w, s, d) of its samples with sigma > 0 (thresholds 0, no stop)."""
    m, recs, _, _ = _sweep(tree, rays, opt)
    out = [([], [], []) for _ in range(m.Q)]
    for a, _, w, s, d, _, _ in recs:
        for q, wi, si, di in zip(a.tolist(), w.tolist(), s.tolist(), d.tolist()):
            out[q][0].append(wi)
            out[q][1].append(si)
            out[q][2].append(di)
    return [tuple(np.asarray(x, dtype=np.float64) for x in r) for r in out]
