#!/usr/bin/env python3
"""grid_weights (svox_t_amd.grid_weights: the HIP march) against the same math written as PyTorch ops on the GPU -- all
rays marched in lock step, the live ones re-gathered every step, scatter_reduce(amax) for the weight and index_add_ for
the count -- on a shell-shaped density volume (a function of the radius: the dense counterpart of synth.shell_tree),
800 x 800 views on a circle around it.  Also: a run-to-run torch.equal of the HIP result.  The PyTorch version is the
same algorithm, not the same bits (its pointwise kernels round differently), so its sample count is printed beside
the HIP one instead of being compared for equality.

    python scripts/grid_weights_timing.py [--reps 10] [--res 128 256] [--views 1 16] [--size 800] [--no-baseline]
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import svox_t_amd as svox                      # noqa: E402
from svox_t_amd import csrc as _C              # noqa: E402
from svox_t_amd.renderer import pinhole_rays   # noqa: E402


def shell_volume(R, dev):
    """sigma(r) > 0 between two radii around the centre of the unit cube, 0 elsewhere"""
    c = (torch.arange(R, device=dev, dtype=torch.float32) + 0.5) / R - 0.5
    r = torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)
    return torch.where((r > 0.30) & (r < 0.38), 30.0 * (1.0 + torch.cos(40.0 * r)) + 5.0, torch.zeros_like(r)).contiguous()


def cameras(V, dev):
    out = []
    for i in range(V):
        a = 2 * math.pi * i / V + 0.3
        eye = torch.tensor([0.5 + 1.6 * math.cos(a), 0.5 + 1.6 * math.sin(a), 0.5 + 0.5 * math.sin(2 * a)], dtype=torch.float64)
        z = eye - 0.5
        z = z / z.norm()
        x = torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64), z)
        x = x / x.norm()
        m = torch.eye(4, dtype=torch.float64)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, torch.linalg.cross(z, x), z, eye
        out.append(m)
    return torch.stack(out).float().to(dev)


def dda(c, inv):
    t1 = -c * inv
    t2 = t1 + inv
    return torch.minimum(t1, t2).amax(-1).clamp_min(0.0), torch.maximum(t1, t2).amin(-1).clamp_max(1e9)


def torch_grid_weights(sigma, origins, dirs, step_size, sigma_thresh):
    """the march of grid_trace_ray for the unit cube (offset 0, scaling 1), every ray at once"""
    R = sigma.shape[0]
    sig = sigma.reshape(-1)
    nrm = dirs.norm(dim=-1, keepdim=True)
    ds = (1.0 / nrm).squeeze(-1)
    d = dirs / nrm
    inv = (1.0 / (d.double() + 1e-9)).float()
    tmin, tmax = dda(origins, inv)
    weight = torch.zeros(R ** 3, device=sigma.device)
    hits = torch.zeros(R ** 3, device=sigma.device)
    live = torch.nonzero(~((tmax < 0) | (tmin > tmax))).squeeze(-1)
    o, d, inv, ds, t, tmax = origins[live], d[live], inv[live], ds[live], tmin[live], tmax[live]
    T = torch.ones_like(t)
    while t.numel():
        pos = (o + t[:, None] * d).clamp(0.0, 1.0 - 1e-6) * R
        fl = pos.floor()
        pos = pos - fl
        u = fl.long().clamp_(0, R - 1)
        cell = (u[:, 0] * R + u[:, 1]) * R + u[:, 2]
        smin, smax = dda(pos, inv)
        delta_t = (smax - smin) / R + step_size
        s = sig[cell]
        m = s > sigma_thresh
        att = torch.where(m, torch.exp(-delta_t * ds * s), torch.ones_like(s))
        w = torch.where(m, T * (1.0 - att), torch.zeros_like(s))
        T = T * att
        weight.scatter_reduce_(0, cell, w, "amax")
        hits.index_add_(0, cell, m.float())
        t = t + delta_t
        keep = torch.nonzero(t < tmax).squeeze(-1)                    # the host read of every step
        if keep.numel() < t.numel():
            o, d, inv, ds, t, tmax, T = o[keep], d[keep], inv[keep], ds[keep], t[keep], tmax[keep], T[keep]
    return weight.reshape(sigma.shape), hits.reshape(sigma.shape)


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--views", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    W = H = a.size
    f = 1.4 * W
    step, thr = 1e-3, 0.01
    for R in a.res:
        sigma = shell_volume(R, dev)
        for V in a.views:
            cams = cameras(V, dev)
            spec, opt = _C.CameraSpec(), _C.RenderOptions()
            spec.c2w, spec.fx, spec.fy, spec.width, spec.height = cams, f, f, W, H
            opt.step_size, opt.sigma_thresh, opt.ndc_width = step, thr, -1
            off, sc = torch.zeros(3, device=dev), torch.ones(3, device=dev)

            def hip():
                return _C.grid_weights(sigma, spec, opt, off, sc)

            t_m, lo_m, hi_m = timed(hip, a.reps)
            r1, r2 = hip(), hip()
            same = all(torch.equal(r1[i], r2[i]) for i in range(2))
            n_hits = int(r1[1].double().sum().item())
            line = (f"R={R} views={V} {W}x{H}: {n_hits} samples in {int((r1[1] > 0).sum().item())} cells | hip {t_m:.3f} ms "
                    f"[{lo_m:.3f}, {hi_m:.3f}]  run-to-run equal {same}")
            if not a.no_baseline:
                rays = [pinhole_rays(c, W, H, f, f) for c in cams]
                o = torch.cat([r[0] for r in rays])
                d = torch.cat([r[1] for r in rays])
                t_t, lo_t, hi_t = timed(lambda: torch_grid_weights(sigma, o, d, step, thr), max(2, a.reps // 5), warm=1)
                ref = torch_grid_weights(sigma, o, d, step, thr)
                line += (f" | torch ops {t_t:.1f} ms [{lo_t:.1f}, {hi_t:.1f}] -> {t_t / t_m:.0f}x  (its samples: {int(ref[1].double().sum().item())}, "
                         f"max |weight diff| {(ref[0] - r1[0]).abs().max().item():.1e})")
            print(line, flush=True)


if __name__ == "__main__":
    main()
