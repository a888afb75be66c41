"""Restatement of the sample faces and of sample_geometry's gradient (include/svoxt.h, svoxt_ray_samples_emit_faces /
svoxt_sample_geometry_bwd / svoxt_sample_weights_bwd_length) on the CPU.

TEST INFRASTRUCTURE ONLY.  The reference has no such operators.  The stepping is tests.depth_restate._March's lock-step
march (oracle/torch_renderer.py's _dda_unit and _locate, float32 in the reference's operation order), walked here once
more because the faces need EVERY crossing, the leaves without a feature row included; its lists are
samples_restate.lists' array for array (tests/test_raygeom_host.py holds that).

    lists_with_faces(tree, rays, opt, min_sigma=None)   FaceLists: the Lists of samples_restate plus, per sample,
                                                  face uint8 = entry | exit << 2, the two planes in WORLD coordinates
                                                  (float64), the lock-step round the crossing was marched in, `first`
                                                  (the ray's first marched crossing) and the ray's tree-space set-up
    geometry_backward32(F, dirs, g_depth, g_length)     (grad_origins, grad_dirs) float32 [Q, 3]: the kernel's sequence, sample
                                                  by sample, every operation rounded to float32
    geometry64(F, origins, dirs, anchored)        (depth, length) float64 torch, the yardstick: autograd through
                                                  z = (P_a - o_a) / d_a with a from the recorded faces and P_a the leaf's
                                                  or cube's plane; anchored: the VALUES are the recorded depth / length
                                                  (z - z.detach() is added), so that what follows sees the lists' numbers
    geometry_bound(F, dirs, g_depth, g_length, step_size)   (bound_origins, bound_dirs) float64 [Q, 3], derived below
    weights64(length, sigma, offsets)             (w, alpha) float64 torch, differentiable in length and sigma
    weights_backward32(length, sigma, offsets, gw, ga)   (grad_sigma, grad_length) float32: the two sweeps of
                                                  samples_restate's docstring, grad_length = sigma * the same bracket
    grad_length_scale(...)                        the tight scale of grad_length: samples_restate.grad_sigma_scale with
                                                  sigma in place of length as the outer factor

THE DEFINITION (float32, per ray in list order, six accumulators from 0; gz_in = g_depth - g_length, gz_out = g_length):
    a = entry;  if a < 3 and d[a] != 0:  u = gz_in  / d[a];  go[a] -= u;  gd[a] -= u * depth
    b = exit;   if b < 3 and d[b] != 0:  v = gz_out / d[b];  go[b] -= v;  gd[b] -= v * (depth + length)

THE BOUND between the definition and the yardstick, per ray and component, summed over the ray's addends in the "tight
scale" manner (every addend priced by its absolute value).  The yardstick's addends are -g / d_a for the
origin and -g z_P / d_a for the direction, z_P = (P_a - o_a) / d_a the plane's own parameter; the definition's are
-g / d_a and -g z / d_a with z the list's depth (or depth + length).  So

  origins   the addends are the same numbers; the definition forms them in float32: one division (2^-24 relative) and
            one rounded subtraction per addend, each at most 2^-24 of the running sum <= the tight sum S_o = sum |g / d_a|:
                bound_o = (n + 1) 2^-24 S_o                                   n: the addends on that accumulator
  dirs      per addend |g| / |d_a| * |z - z_P|, and z - z_P has three parts:
            (1) one step: the march leaves a leaf at its exit plane PLUS step_size, so every depth but that of a ray's
                first marched crossing, and every depth + length, is its plane's parameter plus step_size * delta_scale
                -- the term the definition leaves out on purpose.
            (2) the float32 march against exact arithmetic on the same world numbers, in tree-space units u = 2^-24:
                the origin o_t = fl(offset + fl(scaling o)) and the point p = fl(o_t + fl(t d_t)) are each off by at most
                u (|offset_a| + 2 |o_t,a| + 2) (p lies in [0, 1], |t d_t,a| <= 1 + |o_t,a|); the leaf-local coordinate
                adds at most `levels` roundings of size N u before it is divided by the cell count again (N = 2: none,
                covered by the constant); moving a plane's hit point by e along axis a moves t by e / |d_t,a|:
                    4 u (|offset_a| + 2 |o_t,a| + 4) / |d_t,a|
                the inverse direction is 1 / (d + 1e-9): the chord to the exit, at most sqrt(3) in the unit cube, is off
                by 1e-9 / |d_t,a| of itself, and by 3 u of itself for its three float32 operations:
                    sqrt(3) (1e-9 / |d_t,a| + 3 u)
                and t gathers one rounding of u t per marched crossing, j + 1 of them at lock-step round j, t <= 2 sqrt(3)
                + |o_t| ... priced by the value itself: (j + 2) u |t|.  All of it times delta_scale (z = delta_scale t,
                one more rounding, and delta_scale and d_t carry 4 u relative from the normalisation: 6 u |z| in all).
            (3) the float32 sequence: the division, the product with z, the add depth + length and the subtraction,
                4 roundings of the addend, and n roundings of the running sum: (n + 4) 2^-24 S_d, S_d = sum |g z / d_a|.
                bound_d = sum_addends |g| / |d_a| ((1) + (2)) + (n + 4) 2^-24 S_d
A component without addends has bound 0: it must be exactly 0 on both sides.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from oracle import oracle as O
from oracle.torch_renderer import _dda_unit, _locate
from tests.samples_restate import Lists, _positions

U = 2.0 ** -24
_FACES: list = []       # (tree, origins, dirs, step_size, march): computed once per case, as depth_restate.march keeps its own


class _FaceMarch:
    """depth_restate._March's lock-step march over EVERY crossing, with the two axes of each by the definition of
    include/svoxt.h: crossings[j] = (ray ids, t, delta_t, data word, valid, entry axis, exit axis, entry plane, exit plane)
    -- planes in tree coordinates, float64 (NaN: entry axis 3)."""

    def __init__(self, tree: O.Tree, origins, dirs, step_size):
        f32 = torch.float32
        child = torch.from_numpy(tree.child.reshape(-1))
        data = torch.from_numpy(tree.data.reshape(-1))
        M, N = tree.M, tree.N
        offset = torch.from_numpy(tree.offset.astype(np.float32))
        scaling = torch.from_numpy(tree.scaling.astype(np.float32))
        o = torch.as_tensor(np.asarray(origins), dtype=f32)
        d = torch.as_tensor(np.asarray(dirs), dtype=f32)
        self.Q = Q = o.shape[0]
        o = offset + scaling * o
        d = d * scaling
        nrm = torch.from_numpy(np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).numpy()))
        self.delta_scale = 1.0 / nrm
        d = d * self.delta_scale[:, None]
        inv = (1.0 / (d.double() + 1e-9)).float()
        self.o_t, self.d_t = o, d
        tmin, tmax = _dda_unit(o, inv)
        self.hit = ~((tmax < 0) | (tmin > tmax))
        # the cube's entry axis: n_a = fminf(t1, t2); tmin > 0: the first axis in x, y, z with n_a == tmin, else 3
        t1 = -o * inv
        n = torch.minimum(t1, t1 + inv)
        entry = torch.full((Q,), 3, dtype=torch.int64)
        for a in (2, 1, 0):
            entry = torch.where((tmin > 0) & (n[:, a] == tmin), torch.full_like(entry, a), entry)
        a3 = entry.clamp(max=2)
        plane = torch.where(inv.gather(1, a3[:, None])[:, 0] > 0, 0.0, 1.0).double()          # entering: the near face
        plane = torch.where(entry < 3, plane, torch.full_like(plane, float("nan")))
        self.crossings = []
        ids = torch.nonzero(self.hit).squeeze(1)
        t = tmin[ids].clone()
        first = torch.ones(Q, dtype=torch.bool)
        while ids.numel():
            pos = o[ids] + t[:, None] * d[ids]
            slot, local, cube = _locate(child, N, pos)
            idx = data[slot].long()
            valid = (idx >= 0) & (idx < M)
            iv = inv[ids]
            s_tmin, s_tmax = _dda_unit(local, iv)
            delta_t = (s_tmax - s_tmin) / cube + np.float32(step_size)
            # exit: m_a = fmaxf(-l_a * i_a, -l_a * i_a + i_a); the first axis that holds the minimum, strict-less update
            m1 = -local * iv
            m = torch.maximum(m1, m1 + iv)
            ex = torch.zeros(ids.shape[0], dtype=torch.int64)
            best = m[:, 0]
            for a in (1, 2):
                c = m[:, a] < best
                ex = torch.where(c, torch.full_like(ex, a), ex)
                best = torch.where(c, m[:, a], best)
            # the exit plane in tree coordinates: the far face of the leaf's cell on that axis
            hi = float(np.float32(1.0 - 1e-6))
            pc = pos.clamp(0.0, hi).double()
            cell = torch.round(pc * cube.double()[:, None] - local.double())
            far = (iv > 0).double()
            xplane = ((cell + far) / cube.double()[:, None]).gather(1, ex[:, None])[:, 0]
            self.crossings.append((ids, t, delta_t, idx, valid, entry[ids].clone(), ex, plane[ids].clone(), xplane, first[ids].clone()))
            entry[ids] = ex
            plane[ids] = xplane
            first[ids] = False
            t = t + delta_t
            keep = t < tmax[ids]
            ids, t = ids[keep], t[keep]


def face_march(tree: O.Tree, rays, opt) -> _FaceMarch:
    for tr, org, dr, ss, m in _FACES:
        if tr is tree and org is rays[0] and dr is rays[1] and ss == float(opt.step_size):
            return m
    m = _FaceMarch(tree, rays[0], rays[1], opt.step_size)
    _FACES.append((tree, rays[0], rays[1], float(opt.step_size), m))
    del _FACES[:-8]
    return m


class FaceLists(NamedTuple):
    lists: Lists
    face: np.ndarray          # uint8 [T]
    p_in: np.ndarray          # float64 [T]: the entry plane's world coordinate on the entry axis (NaN: axis 3)
    p_out: np.ndarray         # float64 [T]
    round: np.ndarray         # int64 [T]: the lock-step round (the number of crossings marched before it on its ray)
    first: np.ndarray         # bool [T]: the ray's first marched crossing (its depth is the cube plane's, no step)
    o_t: np.ndarray           # float32 [Q, 3]: the origins in tree space
    d_t: np.ndarray           # float32 [Q, 3]: the unit directions in tree space
    delta_scale: np.ndarray   # float32 [Q]


def lists_with_faces(tree: O.Tree, rays, opt, min_sigma=None) -> FaceLists:
    m = face_march(tree, rays, opt)
    cols = [[] for _ in range(10)]
    for j, cr in enumerate(m.crossings):
        ids, t, delta_t, idx, valid, en, ex, pin, pout, first = cr
        keep = valid.clone()
        if min_sigma is not None:
            sig = torch.from_numpy(tree.features)[idx.clamp(0, tree.M - 1), tree.K - 1]
            keep &= sig > np.float32(min_sigma)
        for c, x in zip(cols, (ids, t, delta_t, idx, en, ex, pin, pout, first, torch.full_like(ids, j))):
            c.append(x[keep])
    if m.crossings:
        ids, t, delta_t, row, en, ex, pin, pout, first, rnd = (torch.cat(c) for c in cols)
    else:
        ids = row = en = ex = rnd = torch.zeros(0, dtype=torch.int64)
        t = delta_t = torch.zeros(0, dtype=torch.float32)
        pin = pout = torch.zeros(0, dtype=torch.float64)
        first = torch.zeros(0, dtype=torch.bool)
    order = torch.sort(ids, stable=True).indices
    ids, t, delta_t, row, en, ex, pin, pout, first, rnd = (x[order] for x in (ids, t, delta_t, row, en, ex, pin, pout, first, rnd))
    ds = m.delta_scale[ids]
    depth = ds * t
    length = delta_t * ds
    offsets = np.zeros(m.Q + 1, dtype=np.int64)
    np.cumsum(np.bincount(ids.numpy(), minlength=m.Q), out=offsets[1:])
    L = Lists(offsets, row.numpy().astype(np.int32), ids.numpy().astype(np.int32), depth.numpy(), length.numpy())
    face = (en | (ex << 2)).numpy().astype(np.uint8)
    off64, sc64 = tree.offset.astype(np.float32).astype(np.float64), tree.scaling.astype(np.float32).astype(np.float64)
    a_in, a_out = en.clamp(max=2).numpy(), ex.numpy()
    p_in = (pin.numpy() - off64[a_in]) / sc64[a_in]              # tree = offset + scaling * world
    p_out = (pout.numpy() - off64[a_out]) / sc64[a_out]
    return FaceLists(L, face, p_in, p_out, rnd.numpy(), first.numpy(), m.o_t.numpy(), m.d_t.numpy(), m.delta_scale.numpy())


def subset(F: FaceLists, index) -> FaceLists:
    """The samples `index` (ascending list positions) as FaceLists over the same rays: what RaySamples.select leaves."""
    index = np.asarray(index)
    L = F.lists
    Q = len(L.offsets) - 1
    offsets = np.zeros(Q + 1, dtype=np.int64)
    np.cumsum(np.bincount(L.ray[index], minlength=Q), out=offsets[1:])
    L2 = Lists(offsets, L.row[index], L.ray[index], L.depth[index], L.length[index])
    return F._replace(lists=L2, face=F.face[index], p_in=F.p_in[index], p_out=F.p_out[index], round=F.round[index], first=F.first[index])


# ------------------------------------------------------------------------------------------- the definition, float32
def geometry_backward32(F: FaceLists, dirs, g_depth, g_length):
    L = F.lists
    f32 = np.float32
    T, Q = L.row.shape[0], len(L.offsets) - 1
    d = np.asarray(dirs, dtype=f32)
    gD = np.zeros(T, f32) if g_depth is None else np.asarray(g_depth, dtype=f32)
    gL = np.zeros(T, f32) if g_length is None else np.asarray(g_length, dtype=f32)
    go, gd = np.zeros((Q, 3), f32), np.zeros((Q, 3), f32)
    with np.errstate(all="ignore"):
        for r, k in _positions(L.offsets):
            r, k = r.numpy(), k.numpy()
            z, ln = L.depth[k], L.length[k]
            gz_in, gz_out = gD[k] - gL[k], gL[k]
            for axis, g, zz in ((F.face[k] & 3, gz_in, z), ((F.face[k] >> 2) & 3, gz_out, z + ln)):      # the entry term first
                a = np.minimum(axis, 2).astype(np.int64)
                da = d[r, a]
                on = (axis < 3) & (da != 0)
                rr, aa = r[on], a[on]
                u = (g[on] / da[on]).astype(f32)
                go[rr, aa] = go[rr, aa] - u                      # (a ray appears once in a round)
                gd[rr, aa] = gd[rr, aa] - (u * zz[on]).astype(f32)
    return go, gd


# ------------------------------------------------------------------------------------------------- the yardstick, float64
def geometry64(F: FaceLists, origins, dirs, anchored=False):
    L = F.lists
    ray = torch.from_numpy(L.ray.astype(np.int64))
    depth_rec = torch.from_numpy(L.depth).double()
    end_rec = torch.from_numpy((L.depth + L.length).astype(np.float32)).double()
    d32 = dirs.detach().to(torch.float32)

    def param(axis, plane, rec):
        a = torch.from_numpy(np.minimum(axis, 2).astype(np.int64))
        oa = origins[ray, a] if len(ray) else origins.new_zeros(0)
        da = dirs[ray, a] if len(ray) else dirs.new_zeros(0)
        on = torch.from_numpy(axis < 3) & (d32[ray, a] != 0)
        safe = torch.where(on, da, torch.ones_like(da))
        z = (torch.from_numpy(np.nan_to_num(plane)) - oa) / safe
        if anchored:
            z = rec + (z - z.detach())
        return torch.where(on, z, rec)

    z_in = param(F.face & 3, F.p_in, depth_rec)
    z_out = param((F.face >> 2) & 3, F.p_out, end_rec)
    return z_in + 0.0, z_out - z_in      # (a node of its own: depth.grad is then d loss / d depth alone, not minus length's share)


def geometry_grad64(F: FaceLists, origins, dirs, g_depth, g_length):
    """(grad_origins, grad_dirs) float64 [Q, 3] of sum(g_depth * depth) + sum(g_length * length) by autograd."""
    o = torch.as_tensor(np.asarray(origins), dtype=torch.float64).clone().requires_grad_(True)
    d = torch.as_tensor(np.asarray(dirs), dtype=torch.float64).clone().requires_grad_(True)
    depth, length = geometry64(F, o, d)
    T = depth.shape[0]
    gD = torch.zeros(T, dtype=torch.float64) if g_depth is None else torch.as_tensor(np.asarray(g_depth), dtype=torch.float64)
    gL = torch.zeros(T, dtype=torch.float64) if g_length is None else torch.as_tensor(np.asarray(g_length), dtype=torch.float64)
    ((depth * gD).sum() + (length * gL).sum() + 0.0 * (o.sum() + d.sum())).backward()
    return o.grad.numpy(), d.grad.numpy()


def geometry_bound(F: FaceLists, dirs, g_depth, g_length, step_size, offset, N=2, levels=0):
    """(bound_origins, bound_dirs) float64 [Q, 3]: the module docstring's derivation, addend by addend."""
    L = F.lists
    T, Q = L.row.shape[0], len(L.offsets) - 1
    d = np.asarray(dirs, dtype=np.float64)
    gD = np.zeros(T) if g_depth is None else np.asarray(g_depth, dtype=np.float64)
    gL = np.zeros(T) if g_length is None else np.asarray(g_length, dtype=np.float64)
    ray = L.ray.astype(np.int64)
    ds = F.delta_scale.astype(np.float64)[ray]
    off = np.abs(np.asarray(offset, dtype=np.float64))
    s_o, s_d, extra, n = (np.zeros((Q, 3)) for _ in range(4))
    z_in, z_out = L.depth.astype(np.float64), (L.depth + L.length).astype(np.float64)
    for axis, g, z, stepped in ((F.face & 3, np.abs(gD - gL), z_in, ~F.first), ((F.face >> 2) & 3, np.abs(gL), z_out, np.ones(T, bool))):
        a = np.minimum(axis, 2).astype(np.int64)
        da = np.abs(d[ray, a])
        on = (axis < 3) & (da != 0)
        r, a, g, z, da = ray[on], a[on], g[on], z[on], da[on]
        dt = np.abs(F.d_t.astype(np.float64)[r, a])
        ot = np.abs(F.o_t.astype(np.float64)[r, a])
        part2 = 4 * U * (off[a] + 2 * ot + 4 + N * levels) / dt + np.sqrt(3.0) * (1e-9 / dt + 3 * U)
        dz = step_size * ds[on] * stepped[on] + ds[on] * part2 + ((F.round[on] + 2) + 6) * U * np.abs(z)
        np.add.at(s_o, (r, a), g / da)
        np.add.at(s_d, (r, a), g / da * np.abs(z))
        np.add.at(extra, (r, a), g / da * dz)
        np.add.at(n, (r, a), 1.0)
    return (n + 1) * U * s_o, extra + (n + 4) * U * s_d


def geometry_tight(F: FaceLists, dirs, abs_in, abs_out):
    """(S_o, S_d) float64 [Q, 3]: sum |g / d_a| and sum |g z / d_a| over a ray's addends for per-sample magnitudes abs_in
    (of gz_in) and abs_out (of gz_out) -- the gradient is linear in the upstream gradients, so an upstream error of that
    size moves grad_origins / grad_dirs by at most this much."""
    L = F.lists
    Q = len(L.offsets) - 1
    d = np.asarray(dirs, dtype=np.float64)
    ray = L.ray.astype(np.int64)
    s_o, s_d = np.zeros((Q, 3)), np.zeros((Q, 3))
    for axis, g, z in ((F.face & 3, abs_in, L.depth.astype(np.float64)), ((F.face >> 2) & 3, abs_out, (L.depth + L.length).astype(np.float64))):
        a = np.minimum(axis, 2).astype(np.int64)
        da = np.abs(d[ray, a])
        on = (axis < 3) & (da != 0)
        np.add.at(s_o, (ray[on], a[on]), np.asarray(g, dtype=np.float64)[on] / da[on])
        np.add.at(s_d, (ray[on], a[on]), np.asarray(g, dtype=np.float64)[on] / da[on] * np.abs(z[on]))
    return s_o, s_d


# --------------------------------------------------------------------------------------- sample_weights in `length`
def weights64(length, sigma, offsets):
    """samples_restate.weights in float64 with `length` a torch tensor too: autograd through both."""
    Q, T = len(offsets) - 1, length.shape[0]
    light = torch.ones(Q, dtype=torch.float64)
    w = torch.zeros(T, dtype=torch.float64)
    pos_all = sigma.detach().to(torch.float32) > 0
    for r, k in _positions(offsets):
        pos = pos_all[k]
        r, k = r[pos], k[pos]
        att = torch.exp(-(length[k] * sigma[k]))
        w = w.index_put((k,), light[r] * (1.0 - att))
        light = light.index_put((r,), light[r] * att)
    return w, 1.0 - light


def weights_backward32(length, sigma, offsets, grad_w, grad_alpha):
    f32 = np.float32
    length, sigma = np.asarray(length, dtype=f32), np.asarray(sigma, dtype=f32)
    T, Q = length.shape[0], len(offsets) - 1
    gw = np.zeros(T, f32) if grad_w is None else np.asarray(grad_w, dtype=f32)
    ga = np.zeros(Q, f32) if grad_alpha is None else np.asarray(grad_alpha, dtype=f32)
    pos = _positions(offsets)
    light, total = np.ones(Q, f32), np.zeros(Q, f32)

    def step(r, k):
        att = O.expf((-(length[k] * sigma[k])).astype(f32))
        wk = (light[r] * (f32(1.0) - att)).astype(f32)
        light[r] = light[r] * att
        return wk

    picks = []
    for r, k in pos:
        r, k = r.numpy(), k.numpy()
        on = sigma[k] > 0
        picks.append((r[on], k[on]))
    for r, k in picks:                                           # sweep 1
        wk = step(r, k)
        total[r] = total[r] + gw[k] * wk
    tail = (ga * light).astype(f32)
    light[:] = 1
    gs, gl = np.zeros(T, f32), np.zeros(T, f32)
    for r, k in picks:                                           # sweep 2: subtract down
        wk = step(r, k)
        total[r] = total[r] - gw[k] * wk
        br = ((gw[k] * light[r]).astype(f32) - total[r]) + tail[r]
        gs[k] = length[k] * br
        gl[k] = sigma[k] * br
    return gs, gl


def grad_length_scale(length, sigma, offsets, grad_w, grad_alpha):
    """[T] float64: sigma_k (|gw_k| T_{k+1} + sum_all_j |gw_j| w_j + |ga| T_end), 0 where sigma <= 0."""
    from tests.samples_restate import grad_sigma_scale
    length = np.asarray(length, dtype=np.float64)
    sigma = np.asarray(sigma, dtype=np.float64)
    s = grad_sigma_scale(length, sigma, offsets, grad_w, grad_alpha)
    with np.errstate(all="ignore"):
        return np.where((sigma > 0) & (length != 0), s / length * sigma, 0.0)
