"""Restatement of the reference's grid_weight_render (svox_t/csrc/rt_kernel.cu:1240-1344: grid_trace_ray +
grid_weight_render_kernel) for the grid_weights tests: numpy float32, every operation rounded as the reference's
float code rounds it, all rays marched in lock step.  The exponential is the oracle's fixed-sequence expf, pixels
come from oracle.camera_rays; the per-cell maximum is taken on the weight's bit pattern as a signed integer and the
count in integers (np.maximum.at / np.add.at), which is what makes both independent of the order of the rays."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from oracle import oracle as O

f32 = np.float32
CLAMP_HI = f32(1.0 - 1e-6)          # clamp_coord: min(1.0 - 1e-6 in double, q), rounded to float (common.cuh:40)
INF = f32(np.inf)


def _dda_unit(c, inv):
    """_dda_unit (rt_kernel.cu:202-218) for points c [n, 3] and inverse directions inv [n, 3] -> (tmin, tmax);
    fminf / fmaxf return the operand that is not a NaN."""
    tmin = np.zeros(len(c), c.dtype)
    tmax = np.full(len(c), 1e9, c.dtype)
    for a in range(3):
        t1 = -c[:, a] * inv[:, a]
        t2 = t1 + inv[:, a]
        tmin = np.fmax(tmin, np.fmin(t1, t2))
        tmax = np.fmin(tmax, np.fmax(t1, t2))
    return tmin, tmax


def march(sigma, origins, dirs, offset, scaling, step_size=1e-3, sigma_thresh=0.0, advance_guard=True, max_steps=None,
          dtype=np.float32):
    """sigma [R, R, R] (or [R, R, R, 1]); world-space origins / dirs [Q, 3] (after any NDC warp); offset, scaling [3].

    Returns weight (float32, shape of sigma), hits (int64, that shape) and, per ray / for the cross-checks with the
    oracle: hit_cube [Q], steps [Q], active [Q], T [Q] (final transmittance), and weight_sum (float64 per cell: the sum
    of the weights, what N3Tree.accumulate_weights means).  advance_guard: t moves through march_advance (a step that
    does not move t ends the march); without it the restatement is the reference's bare `t += delta_t`.

    dtype=np.float64 restates the reference's double instantiation: the same operations in double, except the calls the
    reference makes in float there too -- sqrtf in the norm, expf, and the fmaxf of its atomicMax, which rounds every
    weight to float before it is compared and stored."""
    ft = dtype
    sig = np.ascontiguousarray(np.asarray(sigma, ft))
    shape = sig.shape
    R = shape[0]
    assert shape[:3] == (R, R, R) and sig.size == R ** 3
    sig = sig.reshape(-1)
    Rf = ft(R)
    o = np.asarray(origins, ft).reshape(-1, 3)
    d = np.asarray(dirs, ft).reshape(-1, 3)
    off, sc = np.asarray(offset, ft).reshape(3), np.asarray(scaling, ft).reshape(3)
    step, thr = f32(step_size), f32(sigma_thresh)                        # (RenderOptions holds floats)
    clamp_hi = CLAMP_HI if ft == f32 else np.float64(1.0) - 1e-6
    inf = ft(np.inf)
    Q = len(o)
    with np.errstate(all="ignore"):
        o = off + sc * o                                                 # transform_coord
        d = d * sc                                                       # _get_delta_scale
        nrm = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(f32)).astype(ft)     # sqrtf
        ds = ft(1.0) / nrm
        d = d * ds[:, None]
        inv = (1.0 / (d.astype(np.float64) + 1e-9)).astype(ft)           # invdir, in double
        tmin, tmax = _dda_unit(o, inv)
        hit_cube = ~((tmax < 0) | (tmin > tmax))
        t = tmin.copy()
        T = np.ones(Q, ft)
        steps = np.zeros(Q, np.int64)
        active = np.zeros(Q, np.int64)
        wbits = np.zeros(R ** 3, np.int32)
        hits = np.zeros(R ** 3, np.int64)
        wsum = np.zeros(R ** 3, np.float64)
        n_iter = 0
        while True:
            idx = np.nonzero(hit_cube & (t < tmax))[0]
            if len(idx) == 0:
                break
            n_iter += 1
            assert max_steps is None or n_iter <= max_steps, "the march did not end"
            tt = t[idx]
            pos = o[idx] + tt[:, None] * d[idx]
            pos = np.fmax(ft(0), np.fmin(clamp_hi, pos))                 # clamp_coord
            pos = pos * Rf
            fl = np.floor(pos)
            pos = pos - fl
            uvw = np.clip(fl.astype(np.int64), 0, R - 1)                 # (never clips: the clamped point times R is below R)
            cell = (uvw[:, 0] * R + uvw[:, 1]) * R + uvw[:, 2]
            stmin, stmax = _dda_unit(pos, inv[idx])
            delta_t = (stmax - stmin) / Rf + step
            s = sig[cell]
            m = s > thr                                                  # NaN: no sample
            k = idx[m]
            att = O.expf((-delta_t[m] * ds[k] * s[m]).astype(f32)).astype(ft)        # expf
            w = T[k] * (ft(1) - att)
            T[k] = T[k] * att
            np.maximum.at(wbits, cell[m], np.ascontiguousarray(w.astype(f32)).view(np.int32))      # fmaxf
            np.add.at(hits, cell[m], 1)
            np.add.at(wsum, cell[m], w.astype(np.float64))
            steps[idx] += 1
            active[k] += 1
            tn = tt + delta_t
            t[idx] = np.where(tn > tt, tn, inf) if advance_guard else tn
    return SimpleNamespace(weight=wbits.view(f32).astype(ft).reshape(shape), hits=hits.reshape(shape), hit_cube=hit_cube, steps=steps,
                           active=active, T=T, weight_sum=wsum.reshape(shape), iterations=n_iter)


def march_cameras(sigma, c2w, fx, fy, width, height, offset, scaling, ndc=None, **kw):
    """march() over the pixels of the cameras c2w [V, 3 or 4, 4] (or one matrix): max / sum over all views."""
    ft = kw.get("dtype", f32)
    c2w = np.asarray(c2w, ft)
    if c2w.ndim == 2:
        c2w = c2w[None]
    rays = [O.camera_rays(c, fx, fy, width, height, ndc=ndc, dtype=ft) for c in c2w]
    return march(sigma, np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays]), offset, scaling, **kw)


def look_at(eye, target=(0.5, 0.5, 0.5), up=(0.0, 0.0, 1.0)):
    """float32 [4, 4] camera-to-world matrix of a camera at `eye` looking at `target` (it looks down its -z)."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m.astype(f32)


def shell_sigma(R, seed=0, inner=0.25, outer=0.4, scale=40.0):
    """A dense shell: sigma > 0 between two radii around the cube's centre (noisy, so that no two cells tie), else 0."""
    rng = np.random.default_rng(seed)
    c = (np.arange(R) + 0.5) / R - 0.5
    r = np.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)
    s = np.where((r >= inner) & (r <= outer), scale * (0.25 + rng.random((R, R, R))), 0.0)
    if R < 4:                                                            # (no cell centre of so coarse a grid lies in the shell)
        s = scale * (0.25 + rng.random((R, R, R)))
    return s.astype(f32)


def one_node_tree(sigma):
    """The dense grid as a one-node N3Tree with N = R (R <= 16): (features [R^3, 4] with sigma in the last column,
    data, child)."""
    R = sigma.shape[0]
    feat = np.zeros((R ** 3, 4), f32)
    feat[:, 3] = np.asarray(sigma, f32).reshape(-1)
    return feat, np.arange(R ** 3, dtype=np.int32).reshape(1, R, R, R, 1), np.zeros((1, R, R, R), np.int32)


def full_octree(sigma, empty=1410065408):
    """The dense grid with R = 2^L as a full octree of depth L: leaf (u, v, w) -> feature row (u R + v) R + w.  Takes
    bit-identical steps: scaling by 2 and subtracting the floor are exact.  Returns (features [R^3, 4], data, child)."""
    R = sigma.shape[0]
    L = R.bit_length() - 1
    assert 1 << L == R and L >= 1
    starts = np.cumsum([0] + [8 ** l for l in range(L)])
    n = int(starts[-1])
    child = np.zeros((n, 2, 2, 2), np.int32)
    data = np.full((n, 2, 2, 2, 1), empty, np.int32)
    for l in range(L):
        S = 1 << l
        x, y, z = np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing="ij")
        ids = starts[l] + (x * S + y) * S + z
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    cx, cy, cz = 2 * x + i, 2 * y + j, 2 * z + k
                    if l < L - 1:
                        child[ids, i, j, k] = starts[l + 1] + (cx * 2 * S + cy) * 2 * S + cz - ids
                    else:
                        data[ids, i, j, k, 0] = (cx * R + cy) * R + cz
    feat = np.zeros((R ** 3, 4), f32)
    feat[:, 3] = np.asarray(sigma, f32).reshape(-1)
    return feat, data, child
