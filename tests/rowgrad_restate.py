"""Restatement of the deterministic render backward (include/svoxt.h, svoxt_render_grad_rows_*) in numpy on the CPU.

TEST INFRASTRUCTURE ONLY.  Every sample's contribution to its feature row is formed in float32 in the sequence of the
reference's trace_ray_backward (rt_kernel.cu:331-496) -- the double-precision steps in float64, rounded where the kernel
rounds -- from tests.depth_restate.march (delta_t, delta_scale, row and ray per step), O.expf and O.basis; the sum per
table entry is tests.rows_restate's reduction of those contributions: samples in ascending index (ray index first, then
march order), chunks of 256 from 0, the partials in chunk order.  tests/test_rowgrad_host.py anchors the contributions to
the C++ oracle.

    contributions(tree, rays, opt, g)   Contributions(row int32 [T], ray int32 [T], values float32 [T, K])
    grad(tree, rays, opt, g)            float32 [M, K]: the chunked sums
tree: O.Tree; rays: (origins, dirs, vdirs) numpy; opt: O.RenderOptions; g: float32 [Q, C + 1], or [Q, 1] for the opacity
backward (C = 0)."""
from collections import namedtuple

import numpy as np

from oracle import oracle as O
from tests import depth_restate as D
from tests import rows_restate as R

Contributions = namedtuple("Contributions", "row ray values")
f32, f64 = np.float32, np.float64


def _channels(tree, opt, C, basis, a, ra):
    """e[n, C] = expf(-tmp) per channel for the samples (ray a, row ra): tmp summed from 0 over min_comp .. max_comp."""
    e = np.empty((a.shape[0], C), f32)
    feats = tree.features
    for c in range(C):
        if opt.format != O.FORMAT_RGBA:
            off = c * opt.basis_dim
            tmp = np.zeros(a.shape[0], f32)
            for i in range(opt.min_comp, opt.max_comp + 1):
                tmp = tmp + basis[a, i] * feats[ra, off + i]
            e[:, c] = O.expf(-tmp)
        else:
            e[:, c] = O.expf(-feats[ra, c])
    return e


def contributions(tree: O.Tree, rays, opt, g) -> Contributions:
    g = np.ascontiguousarray(g, f32)
    K, C = tree.K, g.shape[1] - 1
    assert C == 0 or C + 1 == O.out_data_dim(opt, K)
    m = D.march(tree, rays, opt)
    Q = m.Q
    ds_all = m.delta_scale.numpy().astype(f32)
    rgba = opt.format == O.FORMAT_RGBA
    basis = None
    if not rgba and C > 0:
        basis = O.basis(opt.format, opt.basis_dim, rays[2], tree.extra)
    sigma_col = tree.features[:, K - 1]
    bg = f32(opt.background_brightness)
    steps = []
    for ids, _t, delta_t, row in m.steps:
        a, dt, ra = ids.numpy(), delta_t.numpy().astype(f32), row.numpy()
        act = sigma_col[ra] > 0
        if act.any():
            a, dt, ra = a[act], dt[act], ra[act]
            att = O.expf(((-dt) * sigma_col[ra]) * ds_all[a])
            steps.append((a, dt, ra, att, _channels(tree, opt, C, basis, a, ra)))
    with np.errstate(over="ignore", invalid="ignore"):
        # pass 1
        light = np.ones(Q, f32)
        accum = np.zeros(Q, f32)
        for a, dt, ra, att, e in steps:
            weight = light[a] * (f32(1) - att)
            total_color = np.zeros(a.shape[0], f32)
            for c in range(C):
                sig = (1.0 / (1.0 + e[:, c].astype(f64))).astype(f32)
                total_color = total_color + sig * g[a, c]
            light[a] = light[a] * att
            accum[a] = accum[a] + weight * total_color
        total_grad = np.zeros(Q, f32)
        for j in range(C):
            total_grad = total_grad + g[:, j]
        accum = accum + light * bg * total_grad
        light_ray = light.copy()
        # pass 2
        light = np.ones(Q, f32)
        out_ray, out_step, out_row, out_val = [], [], [], []
        for j, (a, dt, ra, att, e) in enumerate(steps):
            n = a.shape[0]
            v = np.zeros((n, K), f32)
            weight = light[a] * (f32(1) - att)
            total_color = np.zeros(n, f32)
            for c in range(C):
                d = 1.0 / (1.0 + e[:, c].astype(f64))
                total_color = (total_color.astype(f64) + d * g[a, c].astype(f64)).astype(f32)
                sig = d.astype(f32)
                if rgba:
                    v[:, c] = weight * sig * (f32(1) - sig) * g[a, c]
                else:
                    gsig = (sig.astype(f64) * (1.0 - sig.astype(f64))).astype(f32)
                    off = c * opt.basis_dim
                    for i in range(opt.min_comp, opt.max_comp + 1):
                        v[:, off + i] = weight * basis[a, i] * gsig * g[a, c]
            light[a] = light[a] * att
            accum[a] = accum[a] - weight * total_color
            ds = ds_all[a]
            v[:, K - 1] = dt * ds * (total_color * light[a] - accum[a]) + dt * ds * g[a, C] * light_ray[a]
            out_ray.append(a)
            out_step.append(np.full(n, j, np.int64))
            out_row.append(ra)
            out_val.append(v)
    if not out_ray:
        return Contributions(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, K), f32))
    ray, step = np.concatenate(out_ray), np.concatenate(out_step)
    order = np.lexsort((step, ray))                              # ray index first, then march order
    return Contributions(np.concatenate(out_row)[order].astype(np.int32), ray[order].astype(np.int32), np.concatenate(out_val)[order])


def grad(tree: O.Tree, rays, opt, g) -> np.ndarray:
    c = contributions(tree, rays, opt, g)
    return R.reduce(c.values, c.row, tree.M, "sum", 0.0).reshape(tree.M, tree.K)
