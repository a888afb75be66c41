#!/usr/bin/env python3
"""The per-sample interface (csrc/svoxt_samples.hip) beside what it stands next to, on the same GPU, tree and rays in one
process per workload, on the two benchmark workloads

    D8: the headline workload (synth depth 8, SH9, K = 28, 800 x 800)
    C4: the config-4 tree (synth depth 9, K = 32, 1024 x 1024)

per workload:
 1. ray_samples(min_sigma = 0) -- two marches, a scan and one host read -- beside render_depth_moments' forward with
    recording (one march): the ratio is recorded, not gated;
 2. sample_weights + accumulate(C = 3), forward + backward (gradients for sigma and values), on those lists, beside the
    same computation in PyTorch ops on the same tensors: the exclusive cumulative sum of length * sigma within each
    ray's segment, exp, index_add for the per-ray sums, autograd for the backward.
    GATE: the HIP pair must not take longer than the PyTorch formulation -- the script exits with status 1 if it does;
 3. the sample total and the longest list.
Every figure is the median of `--reps` event timings of `--batch` steps each, taken after warm-up rounds that go on until
two consecutive rounds agree within 3 %.  Without --only every workload runs in a process of its own and the lines are
written to profiles/samples_timing.txt.

    python scripts/samples_timing.py [--reps 9] [--batch 10] [--only D8]
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
    from svox_t_amd import synth
    depth, K, fmt, W = WORKLOADS.get(name, WARM_UP)
    st = synth.shell_tree(depth)
    feats = synth.shell_features(st.n_features, K, seed=0)
    tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, data_format=fmt, device="cuda")
    r = svox.VolumeRenderer(tree)
    o, d, v = synth.pinhole_rays(W, W, c2w=synth.camera_pose())
    rays = svox.Rays(o.cuda(), d.cuda(), v.cuda())
    f = tree.features
    Q = W * W
    shape = (W, W)

    def lists():
        r.ray_samples(rays, min_sigma=0.0, image_shape=shape)

    def dm_fwd():
        r.render_depth_moments(f, rays, at="entry", image_shape=shape)      # (f requires grad: the samples are recorded)

    t_lists, t_dm = timed(lists, reps, batch), timed(dm_fwd, reps, batch)

    s = r.ray_samples(rays, min_sigma=0.0, image_shape=shape)
    T = len(s)
    sigma = f.detach()[s.row.long(), -1].clone().requires_grad_(True)
    values = torch.sigmoid(f.detach()[s.row.long(), :3]).contiguous().requires_grad_(True)
    g3 = synth.grad_output(Q, 3).cuda()
    ga = synth.grad_output(Q, 1).cuda()[:, 0].contiguous()
    ray = s.ray.long()
    first = s.offsets[ray]                                        # every sample's first of its ray

    def hip_pair():
        sigma.grad = values.grad = None
        w, alpha = svox.sample_weights(s, sigma)
        out = svox.accumulate(s, w, values)
        torch.autograd.backward([out, alpha], [g3, ga])

    def torch_pair():
        sigma.grad = values.grad = None
        x = s.length * sigma
        before = torch.cumsum(x, 0) - x
        seg = before - before[first]
        w = torch.exp(-seg) * (1.0 - torch.exp(-x))
        out = torch.zeros((Q, 3), device=w.device).index_add_(0, ray, w[:, None] * values)
        alpha = torch.zeros((Q,), device=w.device).index_add_(0, ray, w)
        torch.autograd.backward([out, alpha], [g3, ga])

    t_hip, t_torch = timed(hip_pair, reps, batch), timed(torch_pair, reps, batch)
    ok = t_hip <= t_torch
    say(f"{name}: depth {depth}, K = {K}, {W} x {W} rays, M = {f.shape[0]} rows; {T} samples with sigma > 0, "
        f"{T / Q:.1f} a ray, the longest list {int(s.counts.max())}")
    say(f"  ray_samples(min_sigma = 0)                          {t_lists:8.3f} ms")
    say(f"  render_depth_moments forward, recording             {t_dm:8.3f} ms   ray_samples / depth moments = {t_lists / t_dm:.2f}   (not gated)")
    say(f"  sample_weights + accumulate(C = 3), fwd + bwd       {t_hip:8.3f} ms")
    say(f"  the same in PyTorch ops, fwd + bwd                  {t_torch:8.3f} ms   HIP / PyTorch = {t_hip / t_torch:.2f}   "
        f"gate (<= 1): {'holds' if ok else 'FAILS'}")
    return ok


def one_workload(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("samples_timing: needs a GPU (a timing taken anywhere else says nothing)")
    print(f"samples_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}", flush=True)
    run("warm-up", 1, 1, lambda s: None)
    ok = run(args.only, args.reps, args.batch, lambda s: print(s, flush=True))
    sys.exit(0 if ok else GATE_FAILED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "samples_timing.txt"))
    args = ap.parse_args()
    if args.only:
        one_workload(args)
    # one process per workload: this one never opens the GPU
    lines, ok = [], True
    for name in sorted(WORKLOADS, reverse=True):
        cmd = [sys.executable, os.path.abspath(__file__), "--only", name, "--reps", str(args.reps), "--batch", str(args.batch)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode not in (0, GATE_FAILED):
            sys.exit(f"samples_timing: workload {name} ended with status {res.returncode}")
        ok = ok and res.returncode == 0
        out = res.stdout.splitlines()
        lines += out if not lines else out[1:]                    # the header once
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
