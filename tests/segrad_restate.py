"""Restatement of the Gauss-Newton diagonal of se_grad (include/svoxt.h, svoxt_render_hess_rows_*) in numpy on the CPU.

TEST INFRASTRUCTURE ONLY.  Every sample's entry at every column of its feature row is formed in float32 in the sequence the
header writes out -- the double-precision steps in float64, rounded where the kernels round -- from
tests.depth_restate.march (delta_t, delta_scale, row and ray per step), O.expf and O.basis, in the manner of
tests/rowgrad_restate.py; the sum per table entry is tests.rows_restate's reduction: samples in ascending index (ray index
first, then march order), chunks of 256 from 0, the partials in chunk order.  tests/test_segrad_host.py anchors the result
to the float64 Jacobian of oracle.torch_renderer.volume_render.

    contributions(tree, rays, opt, curv)   Contributions(row int32 [T], ray int32 [T], values float32 [T, K])
    hess(tree, rays, opt, curv)            float32 [M, K]: the chunked sums
    scale(tree, rays, opt, curv)           float64 [M, K]: sum over the samples and outputs of |curv| (|a| + |b|)^2, a and b
                                           the two terms of the sigma Jacobian (|jac| alone for a colour column and for
                                           the alpha output): what an entry's rounding error is priced against.  As in
                                           the gradient's tight scale (oracle/svoxt_oracle.cpp, abs_sum_tight), the
                                           suffix sum b = delta (accum_c) is priced by the full sequential sum of pass 1
                                           it is subtracted down from: its float32 error is relative to that sum
    thinnest(tree, rays, opt, curv)        float64 [M]: the smallest 1.f - att among the samples of a row (inf: no sample):
                                           weight = light * (1.f - att) is off by up to 2^-24 / (1 - att) of its value
                                           (att is good to an ulp below 1), which the scale above does not price
tree: O.Tree; rays: (origins, dirs, vdirs) numpy; opt: O.RenderOptions; curv: float32 [Q, C + 1], or [Q, 1] for the opacity
render (C = 0)."""
import numpy as np

from oracle import oracle as O
from tests import depth_restate as D
from tests import rows_restate as R
from tests.rowgrad_restate import Contributions, _channels

f32, f64 = np.float32, np.float64


def _entries(tree: O.Tree, rays, opt, curv, want_scale=False):
    curv = np.ascontiguousarray(curv, f32)
    K, C = tree.K, curv.shape[1] - 1
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
    one = f32(1)
    steps = []
    for ids, _t, delta_t, row in m.steps:
        a, dt, ra = ids.numpy(), delta_t.numpy().astype(f32), row.numpy()
        act = sigma_col[ra] > 0
        if act.any():
            a, dt, ra = a[act], dt[act], ra[act]
            att = O.expf(((-dt) * sigma_col[ra]) * ds_all[a])
            e = _channels(tree, opt, C, basis, a, ra)
            sig = (1.0 / (1.0 + e.astype(f64))).astype(f32)
            steps.append((a, dt, ra, att, sig))
    vals = [np.zeros((s[0].shape[0], K), f32) for s in steps]
    scl = [np.zeros((s[0].shape[0], K), f64) for s in steps]
    with np.errstate(over="ignore", invalid="ignore"):
        # the colour columns: the weight of the sample, the prefix of the gradient's contribution
        light = np.ones(Q, f32)
        for j, (a, dt, ra, att, sig) in enumerate(steps):
            weight = light[a] * (one - att)
            for c in range(C):
                s = sig[:, c]
                if rgba:
                    jac = weight * s * (one - s)
                    vals[j][:, c] = (jac * jac) * curv[a, c]
                    scl[j][:, c] = jac.astype(f64) ** 2 * np.abs(curv[a, c])
                else:
                    gsig = (s.astype(f64) * (1.0 - s.astype(f64))).astype(f32)
                    off = c * opt.basis_dim
                    for i in range(opt.min_comp, opt.max_comp + 1):
                        jac = weight * basis[a, i] * gsig
                        vals[j][:, off + i] = (jac * jac) * curv[a, c]
                        scl[j][:, off + i] = jac.astype(f64) ** 2 * np.abs(curv[a, c])
            light[a] = light[a] * att
        light_ray = light.copy()
        # the sigma column: a two-pass walk per channel, then the alpha output
        h = [np.zeros(s[0].shape[0], f32) for s in steps]
        hs = [np.zeros(s[0].shape[0], f64) for s in steps]
        for c in range(C):
            light = np.ones(Q, f32)
            accum = np.zeros(Q, f32)
            for a, dt, ra, att, sig in steps:                                     # pass 1
                weight = light[a] * (one - att)
                light[a] = light[a] * att
                accum[a] = accum[a] + weight * sig[:, c]
            accum = accum + light * bg
            total = np.abs(accum.astype(f64))                                     # what pass 2 subtracts down from
            light = np.ones(Q, f32)
            for j, (a, dt, ra, att, sig) in enumerate(steps):                     # pass 2
                s = sig[:, c]
                weight = light[a] * (one - att)
                light[a] = light[a] * att
                accum[a] = accum[a] - weight * s
                dd = dt * ds_all[a]
                jac = dd * (s * light[a] - accum[a])
                h[j] = h[j] + (jac * jac) * curv[a, c]
                ab = np.abs(dd.astype(f64)) * (np.abs((s * light[a]).astype(f64)) + total[a])
                hs[j] = hs[j] + ab ** 2 * np.abs(curv[a, c])
        for j, (a, dt, ra, att, sig) in enumerate(steps):
            jac = (dt * ds_all[a]) * light_ray[a]
            h[j] = h[j] + (jac * jac) * curv[a, C]
            vals[j][:, K - 1] = h[j]
            scl[j][:, K - 1] = hs[j] + jac.astype(f64) ** 2 * np.abs(curv[a, C])
    if not steps:
        return Contributions(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, K), f32)), np.zeros((0, K), f64)
    ray = np.concatenate([s[0] for s in steps])
    step = np.concatenate([np.full(s[0].shape[0], j, np.int64) for j, s in enumerate(steps)])
    order = np.lexsort((step, ray))                              # ray index first, then march order
    con = Contributions(np.concatenate([s[2] for s in steps])[order].astype(np.int32), ray[order].astype(np.int32),
                        np.concatenate(vals)[order])
    if want_scale == "thin":
        return con, np.concatenate([(one - s[3]).astype(f64) for s in steps])[order]
    return con, (np.concatenate(scl)[order] if want_scale else None)


def contributions(tree: O.Tree, rays, opt, curv) -> Contributions:
    return _entries(tree, rays, opt, curv)[0]


def hess(tree: O.Tree, rays, opt, curv) -> np.ndarray:
    c = contributions(tree, rays, opt, curv)
    return R.reduce(c.values, c.row, tree.M, "sum", 0.0).reshape(tree.M, tree.K)


def scale(tree: O.Tree, rays, opt, curv) -> np.ndarray:
    c, s = _entries(tree, rays, opt, curv, want_scale=True)
    out = np.zeros((tree.M, tree.K), f64)
    np.add.at(out, c.row, s)
    return out


def thinnest(tree: O.Tree, rays, opt, curv) -> np.ndarray:
    c, t = _entries(tree, rays, opt, curv, want_scale="thin")
    out = np.full(tree.M, np.inf)
    np.minimum.at(out, c.row, t)
    return out
