#!/usr/bin/env python3
"""Sample faces, sample_geometry and sample_weights(length=) (csrc/svoxt_samples.hip) beside the same
computation in PyTorch ops, on the same GPU, lists and tensors in one process per workload, on the two benchmark workloads

    D8: the headline workload (synth depth 8, SH9, K = 28, 800 x 800)
    C4: the config-4 tree (synth depth 9, K = 32, 1024 x 1024)

per workload, on the lists of ray_samples(min_sigma = 0, faces = True):
 (a) sample_geometry's backward (one kernel, a lane per ray) beside the per-sample terms as element-wise ops on [T]
     tensors with gathered dirs, then four index_put_(accumulate=True) into two [Q, 3] tensors.        GATE: HIP <= PyTorch
 (b) sample_weights(length=) + accumulate(C = 3), forward + backward with gradients for sigma, length and values, beside
     scripts/samples_timing.py's composition in PyTorch ops (segmented cumulative sum, exp, index_add, autograd) with
     length.requires_grad.                                                                              GATE: HIP <= PyTorch
 not gated: ray_samples(faces=True) beside faces=False; the pose-refinement chain -- pinhole_rays(c2w) -> ray_samples(
     faces=True) -> sample_geometry -> sample_weights(length=) -> accumulate(w, depth), forward + backward to c2w.grad --
     beside render_depth_moments forward + backward (the gradient of the same loss in the feature table).
The script exits with status 1 if a gate fails.  Every figure is the median of `--reps` event timings of `--batch` steps
each, taken after warm-up rounds that go on until two consecutive rounds agree within 3 %.  Without --only every workload
runs in a process of its own, under its own time limit, and the lines are written to profiles/raygeom_timing.txt.

    python scripts/raygeom_timing.py [--reps 9] [--batch 10] [--only D8]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"D8": (8, 28, "SH9", 800), "C4": (9, 32, "RGBA", 1024)}
WARM_UP = (5, 28, "SH9", 64)
GATE_FAILED = 3
LIMIT_S = 400                                   # a workload's process


def round_of(fn, batch):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / batch


def timed(fn, reps, batch):
    last = round_of(fn, batch)
    for _ in range(20):                         # warm up until converged
        cur = round_of(fn, batch)
        ok = abs(cur - last) <= 0.03 * last
        last = cur
        if ok:
            break
    ts = sorted(round_of(fn, batch) for _ in range(reps))
    return ts[len(ts) // 2]


def torch_geometry_backward(s, dirs, g_depth, g_length):
    """sample_geometry's backward in PyTorch ops: the sums come out in the order of the atomics."""
    import torch
    Q = s.Q
    ray = s.ray.long()
    a, b = (s.face & 3).long(), ((s.face >> 2) & 3).long()
    ac = a.clamp(max=2)
    da, db = dirs[ray, ac], dirs[ray, b]
    zero = torch.zeros_like(g_depth)
    u = torch.where((a < 3) & (da != 0), (g_depth - g_length) / da, zero)
    v = torch.where(db != 0, g_length / db, zero)
    go = torch.zeros((Q, 3), device=dirs.device).index_put_((ray, ac), -u, accumulate=True).index_put_((ray, b), -v, accumulate=True)
    gd = torch.zeros((Q, 3), device=dirs.device).index_put_((ray, ac), -(u * s.depth), accumulate=True)
    gd.index_put_((ray, b), -(v * (s.depth + s.length)), accumulate=True)
    return go, gd


def run(name, reps, batch, say):
    import numpy as np
    import torch
    import svox_t_amd as svox
    from svox_t_amd import synth
    from svox_t_amd.csrc import _extras as X
    from svox_t_amd.renderer import pinhole_rays
    depth, K, fmt, W = WORKLOADS.get(name, WARM_UP)
    st = synth.shell_tree(depth)
    feats = synth.shell_features(st.n_features, K, seed=0)
    tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, data_format=fmt, device="cuda")
    r = svox.VolumeRenderer(tree)
    o, d, v = synth.pinhole_rays(W, W, c2w=synth.camera_pose())
    rays = svox.Rays(o.cuda(), d.cuda(), v.cuda())
    f = tree.features
    Q, shape = W * W, (W, W)

    t_plain = timed(lambda: r.ray_samples(rays, min_sigma=0.0, image_shape=shape), reps, batch)
    t_faces = timed(lambda: r.ray_samples(rays, min_sigma=0.0, image_shape=shape, faces=True), reps, batch)
    s = r.ray_samples(rays, min_sigma=0.0, image_shape=shape, faces=True)
    T = len(s)
    ray = s.ray.long()

    # (a) the geometry backward
    g_depth = synth.grad_output(T, 1, seed=2).cuda()[:, 0].contiguous()
    g_length = synth.grad_output(T, 1, seed=3).cuda()[:, 0].contiguous()
    t_geo = timed(lambda: X.sample_geometry_backward(s.offsets, s.face, s.depth, s.length, rays.dirs, g_depth, g_length), reps, batch)
    t_geo_torch = timed(lambda: torch_geometry_backward(s, rays.dirs, g_depth, g_length), reps, batch)
    go, gd = X.sample_geometry_backward(s.offsets, s.face, s.depth, s.length, rays.dirs, g_depth, g_length)
    go_t, gd_t = torch_geometry_backward(s, rays.dirs, g_depth, g_length)
    apart = max(float((go - go_t).abs().max() / go_t.abs().max()), float((gd - gd_t).abs().max() / gd_t.abs().max()))

    # (b) sample_weights(length=) + accumulate, forward + backward with three gradients
    sigma = f.detach()[s.row.long(), -1].clone().requires_grad_(True)
    length = s.length.clone().requires_grad_(True)
    values = torch.sigmoid(f.detach()[s.row.long(), :3]).contiguous().requires_grad_(True)
    g3 = synth.grad_output(Q, 3).cuda()
    ga = synth.grad_output(Q, 1).cuda()[:, 0].contiguous()
    first = s.offsets[ray]                                        # every sample's first of its ray

    def hip_pair():
        sigma.grad = values.grad = length.grad = None
        w, alpha = svox.sample_weights(s, sigma, length=length)
        out = svox.accumulate(s, w, values)
        torch.autograd.backward([out, alpha], [g3, ga])

    def torch_pair():
        sigma.grad = values.grad = length.grad = None
        x = length * sigma
        before = torch.cumsum(x, 0) - x
        seg = before - before[first]
        w = torch.exp(-seg) * (1.0 - torch.exp(-x))
        out = torch.zeros((Q, 3), device=w.device).index_add_(0, ray, w[:, None] * values)
        alpha = torch.zeros((Q,), device=w.device).index_add_(0, ray, w)
        torch.autograd.backward([out, alpha], [g3, ga])

    t_hip, t_torch = timed(hip_pair, reps, batch), timed(torch_pair, reps, batch)

    # not gated: the chain to c2w.grad beside the depth moments' forward + backward
    pose = torch.from_numpy(synth.camera_pose().astype(np.float32)).cuda()
    fx = 1111.111 * W / 800.0
    g1 = synth.grad_output(Q, 1, seed=4).cuda()[:, 0].contiguous()
    sig_of = f.detach()[:, -1].contiguous()

    def chain():
        c2w = pose.clone().requires_grad_(True)
        oo, dd, vv = pinhole_rays(c2w, W, W, fx, fx)
        rr = svox.Rays(oo, dd, vv)
        ss = r.ray_samples(rr, min_sigma=0.0, image_shape=shape, faces=True)
        z, ln = svox.sample_geometry(ss, rr)
        w, alpha = svox.sample_weights(ss, sig_of[ss.row.long()], length=ln)
        out = svox.accumulate(ss, w, z[:, None])
        torch.autograd.backward([out[:, 0], alpha], [g1, ga])
        return c2w.grad

    g3m = torch.stack([g1, torch.zeros_like(g1), ga], dim=1).contiguous()

    def moments():
        f.grad = None
        r.render_depth_moments(f, rays, at="entry", image_shape=shape).backward(g3m)

    t_chain, t_dm = timed(chain, reps, batch), timed(moments, reps, batch)
    same = torch.equal(chain(), chain())

    ok_a, ok_b = t_geo <= t_geo_torch, t_hip <= t_torch
    say(f"{name}: depth {depth}, K = {K}, {W} x {W} rays; {T} samples with sigma > 0, {T / Q:.1f} a ray, the longest list {int(s.counts.max())}")
    say(f"  (a) sample_geometry backward (grad_origins, grad_dirs)            {t_geo:8.3f} ms")
    say(f"      element-wise terms + 4 index_put_(accumulate)                 {t_geo_torch:8.3f} ms   HIP / PyTorch = {t_geo / t_geo_torch:.2f}   "
        f"gate (<= 1): {'holds' if ok_a else 'FAILS'}   (apart by {apart:.1e} of the largest entry: the order of the atomics)")
    say(f"  (b) sample_weights(length=) + accumulate(C = 3), fwd + bwd         {t_hip:8.3f} ms")
    say(f"      the same in PyTorch ops, fwd + bwd                            {t_torch:8.3f} ms   HIP / PyTorch = {t_hip / t_torch:.2f}   "
        f"gate (<= 1): {'holds' if ok_b else 'FAILS'}")
    say(f"  ray_samples(min_sigma = 0), faces=False / faces=True              {t_plain:8.3f} / {t_faces:8.3f} ms   faces / plain = {t_faces / t_plain:.2f}   (not gated)")
    say(f"  the chain c2w -> rays -> lists -> geometry -> weights -> depth, fwd + bwd  {t_chain:8.3f} ms   (c2w.grad twice the same bits: {same})")
    say(f"  render_depth_moments, fwd + bwd (the feature table's gradient)    {t_dm:8.3f} ms   chain / depth moments = {t_chain / t_dm:.2f}   (not gated)")
    return ok_a and ok_b


def one_workload(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("raygeom_timing: needs a GPU (a timing taken anywhere else says nothing)")
    print(f"raygeom_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}", flush=True)
    run("warm-up", 1, 1, lambda s: None)
    ok = run(args.only, args.reps, args.batch, lambda s: print(s, flush=True))
    sys.exit(0 if ok else GATE_FAILED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raygeom_timing.txt"))
    args = ap.parse_args()
    if args.only:
        one_workload(args)
    # one process per workload, each under its own time limit: this one never opens the GPU
    lines, ok = [], True
    for name in sorted(WORKLOADS, reverse=True):
        cmd = [sys.executable, os.path.abspath(__file__), "--only", name, "--reps", str(args.reps), "--batch", str(args.batch)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            sys.exit(f"raygeom_timing: workload {name} ran into its limit of {LIMIT_S} s; nothing more is started")
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode not in (0, GATE_FAILED):
            sys.exit(f"raygeom_timing: workload {name} ended with status {res.returncode}; nothing more is started")
        ok = ok and res.returncode == 0
        out = res.stdout.splitlines()
        lines += out if not lines else out[1:]                    # the header once
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
