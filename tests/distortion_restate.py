"""Restatement of render_distortion (include/svoxt.h, svoxt_distortion_fwd / _bwd) as a CPU lock-step march in torch.

TEST INFRASTRUCTURE ONLY.  The reference has no such operator, so this file is what the HIP kernels are held to; it is
tied to the C++ oracle at two points (tests/test_distortion_host.py) -- its alpha column has the bits of
O.opacity_render, and its gradient for grad_output (0, ga) is O.volume_render_backward's with a one-column grad_output
-- and to the loss's definition, the O(n^2) sum over pairs, at a third.

The march is tests/depth_restate.py's (the oracle's stepping in float32: the same leaves are visited).  Compositing runs
in `dtype`: float32 reproduces the kernels' operation sequence, float64 is the yardstick for tolerances and gradients.

    distortion(tree, rays, opt, dtype)          [Q, 2] (L, alpha)
    distortion_grad(tree, rays, opt, g)         [M, K] float64: autograd of sum(distortion * g) at thresholds 0
    distortion_grad_scale(tree, rays, opt, g)   [M, K] float64: sum_k d_k (|gd| (|u_k| T_{k+1} + 2 L + 2 E_0 + ETA V_k) +
                                                |ga| T_end), the gradient's addends priced one by one, the suffix sum by
                                                the full sum 2 L and E_k by the E_0 they are subtracted down from, and one
                                                unit in the last place of every attenuation (the function's docstring)
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


ETA = 2.0 ** -23 / 1e-5          # one unit in the last place of an attenuation, in units of the bound 1e-5 * scale


def distortion_grad_scale(tree: O.Tree, rays, opt, grad_output):
    """[M, K] float64, non-zero in the sigma column only: sum over the samples of a row of
    d_k (|gd| (|u_k| T_{k+1} + 2 L + 2 E_0 + ETA V_k) + |ga| T_end), u_k = 2 (D_k + E_k) + (2/3) w_k d_k.

    |u_k| T_{k+1} + 2 L prices the addends of u_k T_{k+1} - sum_{i>k} w_i u_i as they stand.  Two rounding errors of the
    float32 sequence are proportional to neither, and the other two terms price them:

    2 E_0.  Sweep 2 does not sum E_k = sum_{j>k} w_j (s_j - s_k), it subtracts it down from E_0 = sum_j w_j (s_j - s_0):
        E_k = E_{k-1} - (A_tot - A_k)(s_k - s_{k-1}).  Every intermediate lies in [E_k, E_0], so E_k carries an error of
        a few units in the last place of E_0 whatever its own size -- behind a thin first sample E_0 is the ray's whole
        spread while E_k, u_k and 2 L = sum w_i u_i >= 2 w_0 E_0 are all small.  u_k = 2 (D_k + E_k) + ... moves by twice
        that error; it enters the sample's value once through u_k T_{k+1} and once, times w_i for every i <= k, through
        the suffix sum: 2 E_0 (T_{k+1} + sum_{i<=k} w_i) = 2 E_0.
    ETA V_k, V_k = 2 sum_j T_j |s_k - s_j| + (2/3) d_k T_k.  att_j is a float32 exponential: it is off by up to one unit
        in its last place, 2^-23 att_j at most, and so is w_j = T_j (1 - att_j) in absolute terms, by 2^-23 T_j -- of a thin
        sample's weight, 1 - att_j ~ 1e-3, that is 1e-4, where the float64 yardstick has the exact exponential.  (T_j
        itself is off by as much relative to T_j: that is priced with the addends it multiplies.)  u_k moves by
        2 sum_j dw_j |s_k - s_j| + (2/3) d_k dw_k <= 2^-23 V_k, and reaches the value as 2 E_0 does, with total weight 1.
        An error of fixed absolute size enters a scale that is multiplied by 1e-5 divided by 1e-5: ETA = 2^-23 / 1e-5.

    On coherent camera rays over a shell (w_0 is no thinner than the rest) 2 L already covers both; on irregular trees
    with sigma from 1e-2 to 1e4 along one ray it does not (tests/test_gpu_adversarial.py)."""
    m, recs, L, t_end = _sweep(tree, rays, opt)
    g = torch.as_tensor(np.asarray(grad_output), dtype=torch.float64).abs()
    Q = m.Q
    zeros = lambda: torch.zeros(Q, dtype=torch.float64)              # noqa: E731
    # forward: E_0, and P_k = sum_{j<k} T_j (s_k - s_j) as D_k is formed, with T_j (in front of sample j) in the place of w_j
    s0, E0, B, P, sp = zeros(), zeros(), zeros(), zeros(), zeros()
    seen = torch.zeros(Q, dtype=torch.bool)
    before = []
    for a, ra, w, s, d, Dk, tn in recs:
        s0[a] = torch.where(seen[a], s0[a], s)
        seen[a] = True
        E0[a] += w * (s - s0[a])
        P[a] += B[a] * (s - sp[a])                                   # (the first sample: B == 0)
        sp[a] = s
        B[a] += tn + w
        before.append(P[a].clone())
    after = zeros()                                                  # sum_{j>k} w_j
    E = zeros()                                                      # sum_{j>k} w_j (s_j - s_k)
    C, R = zeros(), zeros()                                          # sum_{j>k} T_j and sum_{j>k} T_j (s_j - s_k)
    sn = zeros()                                                     # s_{k+1}
    scale = np.zeros((tree.M, tree.K), dtype=np.float64)
    for (a, ra, w, s, d, Dk, tn), Pk in zip(reversed(recs), reversed(before)):
        E[a] += after[a] * (sn[a] - s)                               # (the last sample: after == 0)
        R[a] += C[a] * (sn[a] - s)
        u = 2.0 * (Dk + E[a]) + (2.0 / 3.0) * w * d
        V = 2.0 * (Pk + R[a]) + (2.0 / 3.0) * d * (tn + w)
        np.add.at(scale[:, tree.K - 1], ra.numpy(),
                  (d * (g[a, 0] * (u.abs() * tn + 2.0 * L[a] + 2.0 * E0[a] + ETA * V) + g[a, 1] * t_end[a])).numpy())
        after[a] += w
        C[a] += tn + w
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
