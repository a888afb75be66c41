#!/usr/bin/env python3
"""N3Tree.interp (csrc/svoxt_interp.hip) beside the same computation in PyTorch ops, on the same GPU, tree and points in
one process per workload, on the two benchmark workloads

    D8: the headline workload (synth depth 8, SH9, K = 28, 800 x 800)
    C4: the config-4 tree (synth depth 9, K = 32, 1024 x 1024)

The points are the mid-points of ray_samples(min_sigma = 0): RaySamples.points(rays).  Per workload:
 (a) interp forward + table backward on all K columns FROM THE POINTS, every step: the stencil, the value, the row plan of
     the 8 Q entries (its sort and its one host read) and the gradient.                              GATE: HIP <= PyTorch
     The PyTorch form: the leaf of every point (forward's node ids), its corner (snap), depth and size (leaf_boxes'
     arithmetic), the eight lattice points, ONE tree.forward over the 8 Q points with its backward, the weights and the
     weighted sum as torch ops with autograd.
 (b) the same with the stencil and its plan kept (a second table, a second step over the same points): interp_rows
     forward + backward.  Reported beside the same PyTorch figure, not gated.
 not gated: the forward alone (stencil + value), the stencil alone, the sigma column only (dim = -1, warm), the point
 gradient, the plan build.
The script exits with status 1 if the gate fails.  Every figure is the median of `--reps` event timings of `--batch`
steps each, taken after warm-up rounds that go on until two consecutive rounds agree within 3 %.  Without --only every
workload runs in a process of its own, under its own time limit, and the lines are written to
profiles/interp_timing.txt.

    python scripts/interp_timing.py [--reps 9] [--batch 10] [--only D8]
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
LIMIT_S = 500                                   # a workload's process


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


def run(name, reps, batch, say):
    import torch
    import svox_t_amd as svox
    import svox_t_amd.csrc as _C
    from svox_t_amd import synth
    depth, K, fmt, W = WORKLOADS.get(name, WARM_UP)
    st = synth.shell_tree(depth)
    feats = synth.shell_features(st.n_features, K, seed=0)
    tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, data_format=fmt, device="cuda")
    r = svox.VolumeRenderer(tree)
    o, d, v = synth.pinhole_rays(W, W, c2w=synth.camera_pose())
    rays = svox.Rays(o.cuda(), d.cuda(), v.cuda())
    s = r.ray_samples(rays, min_sigma=0.0, image_shape=(W, W))
    pts = s.points(rays).contiguous()
    Q = pts.shape[0]
    M = tree.features.shape[0]
    N = tree.N
    f = tree.features.detach().clone().requires_grad_(True)
    g = synth.grad_output(Q, K).cuda().contiguous()
    corner_bits = torch.tensor([[(j >> 2) & 1, (j >> 1) & 1, j & 1] for j in range(8)], dtype=torch.float32, device="cuda")

    def hip_cold():
        f.grad = None
        tree.interp(pts, features=f).backward(g)

    kept = tree.interp_stencil(pts)
    kept.row_plan(M)

    def hip_warm():
        f.grad = None
        svox.interp_rows(kept, f).backward(g)

    def hip_sigma():
        f.grad = None
        svox.interp_rows(kept, f, dim=-1).backward(g[:, :1])

    def hip_forward():
        with torch.no_grad():
            tree.interp(pts, features=f)

    def hip_stencil():
        tree.interp_stencil(pts)

    def hip_plan():
        _C.row_plan(kept.rows.reshape(-1), M)

    spec = tree._spec(f.detach())

    def hip_points():
        _C._extras.interp_points_bwd(spec, pts, kept.rows, f.detach(), g, None)

    def torch_form():
        f.grad = None
        with torch.no_grad():
            _, slot = tree.forward(f.detach(), pts, want_node_ids=True)
            dep = tree.parent_depth[slot // (N ** 3), 1]
            length = (float(N) ** (-dep.float() - 1.0))[:, None] / tree.invradius
            centre = tree.snap(pts) + 0.5 * length
            u = (pts - centre) / length
            sgn = torch.where(u < 0, -1.0, 1.0)
            fr = u.abs()
            X = centre[:, None, :] + corner_bits[None, :, :] * (sgn * length)[:, None, :]
            m = torch.where(corner_bits[None, :, :] > 0, fr[:, None, :], 1.0 - fr[:, None, :])
            w = m[:, :, 0] * m[:, :, 1] * m[:, :, 2]
            t = tree.world2tree(X)
            inside = ((t >= 0) & (t < 1)).all(dim=2, keepdim=True)
            X = torch.where(inside, X, centre[:, None, :])                  # fill = "self": the own leaf
        vals = tree.forward(f, X.reshape(-1, 3))
        out = (w[:, :, None] * vals.view(Q, 8, K)).sum(dim=1)
        out.backward(g)

    t_cold, t_torch = timed(hip_cold, reps, batch), timed(torch_form, reps, batch)
    t_warm, t_sigma = timed(hip_warm, reps, batch), timed(hip_sigma, reps, batch)
    t_fwd, t_st, t_plan, t_pts = (timed(x, reps, batch) for x in (hip_forward, hip_stencil, hip_plan, hip_points))
    ok = t_cold <= t_torch
    plan = kept.row_plan(M)
    say(f"{name}: depth {depth}, K = {K}, {W} x {W} rays; {Q} points (the mid-points of the samples with sigma > 0), {M} rows; "
        f"8 Q = {8 * Q} entries, the longest row {plan.longest}, {plan.long_rows.shape[0]} long rows")
    say(f"  (a) interp from the points, fwd + table bwd, plan built every step   {t_cold:9.3f} ms")
    say(f"      PyTorch: lattice points, one forward over 8 Q, weighted sum, bwd  {t_torch:9.3f} ms   HIP / PyTorch = {t_cold / t_torch:.2f}   "
        f"gate (<= 1): {'holds' if ok else 'FAILS'}")
    say(f"  (b) interp_rows over a kept stencil and plan, fwd + table bwd         {t_warm:9.3f} ms   HIP / PyTorch = {t_warm / t_torch:.2f}   (not gated)")
    say(f"  forward alone (stencil + value)                                      {t_fwd:9.3f} ms   (not gated)")
    say(f"  stencil alone                                                        {t_st:9.3f} ms   (not gated)")
    say(f"  sigma column only (dim = -1), kept stencil, fwd + bwd                 {t_sigma:9.3f} ms   (not gated)")
    say(f"  point gradient (interp_points_bwd)                                   {t_pts:9.3f} ms   (not gated)")
    say(f"  plan build over 8 Q entries (sort, one host read)                    {t_plan:9.3f} ms   plan / (a) = {t_plan / t_cold:.2f}   (not gated)")
    return ok


def one_workload(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("interp_timing: needs a GPU (a timing taken anywhere else says nothing)")
    print(f"interp_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}", flush=True)
    run("warm-up", 1, 1, lambda s: None)
    ok = run(args.only, args.reps, args.batch, lambda s: print(s, flush=True))
    sys.exit(0 if ok else GATE_FAILED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp_timing.txt"))
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
            sys.exit(f"interp_timing: workload {name} ran into its limit of {LIMIT_S} s; nothing more is started")
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode not in (0, GATE_FAILED):
            sys.exit(f"interp_timing: workload {name} ended with status {res.returncode}; nothing more is started")
        ok = ok and res.returncode == 0
        out = res.stdout.splitlines()
        lines += out if not lines else out[1:]                    # the header once
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
