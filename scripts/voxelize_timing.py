#!/usr/bin/env python3
"""voxelize (svox_t_amd.voxelize: the HIP gather) against the same math written in plain PyTorch float32 (enumerated
window offsets, a mask, index_add_ -- what a user of this package wrote before), forward and forward+backward (both
gradients), and a run-to-run torch.equal check of the HIP forward and backward.

    S1: 1 000 000 points on a noisy sphere shell in the unit cube, n = 256, kernel_radius 1 voxel, conv_radius 2 voxels
    S2: S1 with 25 % of the points inside one 4-voxel cluster
    S3: 200 000 points, n = 128, conv_radius 6 voxels (kernel_radius 2 voxels)

    python scripts/voxelize_timing.py [--reps 10] [--no-baseline]
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import svox_t_amd as svox                      # noqa: E402
from svox_t_amd import csrc as _C              # noqa: E402


def cloud(P, cluster_frac, seed, n):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    pts = 0.5 + 0.35 * (1.0 + 0.05 * torch.randn(P, 1, generator=g)) * d
    k = int(P * cluster_frac)
    if k:
        sel = torch.randperm(P, generator=g)[:k]
        vs = 1.0 / (n - 1)
        pts[sel] = 0.3 + 4 * vs * torch.rand(k, 3, generator=g)          # one 4-voxel cube
    return pts.float()


def torch_voxelize(points, feats, corner, size, n, kr, cr):
    """the reference's p2v in PyTorch: every offset of the window around each point, masked, index_add_"""
    c = torch.tensor(corner, device=points.device)
    vs = torch.tensor(size, device=points.device) / (n - 1)
    lo = torch.floor((points - cr - c) / vs)
    R = int(math.ceil(cr / float(vs.min()))) + 1
    rng = torch.arange(0, 2 * R + 1, device=points.device)
    offs = torch.stack(torch.meshgrid(rng, rng, rng, indexing="ij"), -1).reshape(-1, 3)
    hi = torch.ceil((points + cr - c) / vs).clamp(0, n - 1)
    lo = lo.clamp(0, n - 1)
    out = torch.zeros(n ** 3, device=points.device)
    sigma = feats[:, -1]
    for b in range(0, offs.shape[0], 27):
        v = lo[:, None, :] + offs[None, b:b + 27]                        # [P, B, 3]
        inside = (v <= hi[:, None, :]).all(-1)
        d = points[:, None, :] - (v * vs + c)
        r = torch.sqrt((d * d).sum(-1))
        m = inside & (r <= cr)
        w = torch.exp(-r * r / (2 * kr * kr)) * sigma[:, None] * m
        idx = ((v[..., 0] * n + v[..., 1]) * n + v[..., 2]).long().clamp(0, n ** 3 - 1)
        out = out.index_add(0, idx.reshape(-1), w.reshape(-1))
    return out.reshape(n, n, n, 1)


def timed(fn, reps):
    for _ in range(2):
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
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cases = [("S1", 1_000_000, 0.0, 256, 1.0, 2.0), ("S2", 1_000_000, 0.25, 256, 1.0, 2.0),
             ("S3", 200_000, 0.0, 128, 2.0, 6.0)]
    for name, P, frac, n, krv, crv in cases:
        vs = 1.0 / (n - 1)
        kr, cr = krv * vs, crv * vs
        pts = cloud(P, frac, 0, n).to(dev)
        feats = torch.rand(P, 1, device=dev) + 0.5
        args = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), n, kr, cr)
        p = pts.clone().requires_grad_(True)
        f = feats.clone().requires_grad_(True)

        def fwd():
            with torch.no_grad():
                return svox.voxelize(pts, feats, *args)

        def fwd_bwd():
            svox.voxelize(p, f, *args).sum().backward()

        t_f, t_fb = timed(fwd, a.reps), timed(fwd_bwd, a.reps)
        v1, v2 = fwd(), fwd()
        go = torch.randn(n, n, n, 1, device=dev)
        g1 = _C.p2v_backward(go, pts, feats, *args)
        g2 = _C.p2v_backward(go, pts, feats, *args)
        same = torch.equal(v1, v2) and torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])
        line = f"{name}: P={P} n={n} cr={crv:g}vx kr={krv:g}vx  hip fwd {t_f:.3f} ms  fwd+bwd {t_fb:.3f} ms  run-to-run equal {same}"
        if not a.no_baseline:
            def b_fwd():
                with torch.no_grad():
                    return torch_voxelize(pts, feats, *args)

            def b_fwd_bwd():
                torch_voxelize(p, f, *args).sum().backward()

            bt_f, bt_fb = timed(b_fwd, max(2, a.reps // 4)), timed(b_fwd_bwd, max(2, a.reps // 4))
            ref = b_fwd()
            err = ((v1 - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()
            line += (f"  | torch fwd {bt_f:.3f} ms  fwd+bwd {bt_fb:.3f} ms  -> {bt_f / t_f:.1f}x / {bt_fb / t_fb:.1f}x"
                     f"  (max |diff| / max = {err:.1e})")
        print(line, flush=True)


if __name__ == "__main__":
    main()
