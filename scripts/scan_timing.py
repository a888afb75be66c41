#!/usr/bin/env python3
"""ray_scan, ray_quantile and RaySamples.select (csrc/svoxt_scan.hip) beside the same computation in PyTorch ops, on the
same GPU, lists and tensors in one process per workload, on the two benchmark workloads

    D8: the headline workload (synth depth 8, SH9, K = 28, 800 x 800)
    C4: the config-4 tree (synth depth 9, K = 32, 1024 x 1024)

per workload, on the lists of ray_samples(min_sigma = 0) and their compositing weights w:
 (a) ray_scan(w, "sum"), forward + backward, beside the global torch.cumsum minus the value gathered at each ray's start
     through `ray`, with autograd.                                                                      GATE: HIP <= PyTorch
 (b) select(keep) with about half the samples kept, beside nonzero + five index-selects + the per-ray counts of the kept
     samples (index_add) and their cumsum for the offsets.                                              GATE: HIP <= PyTorch
 not gated: ray_scan "prod" and "max" forward + backward, ray_quantile with nq = 3, select beside ray_samples.
The script exits with status 1 if a gate fails.  Every figure is the median of `--reps` event timings of `--batch` steps
each, taken after warm-up rounds that go on until two consecutive rounds agree within 3 %.  Without --only every workload
runs in a process of its own, under its own time limit, and the lines are written to profiles/scan_timing.txt.

    python scripts/scan_timing.py [--reps 9] [--batch 10] [--only D8]
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
    f = tree.features.detach()
    Q, shape = W * W, (W, W)

    def lists():
        r.ray_samples(rays, min_sigma=0.0, image_shape=shape)

    t_lists = timed(lists, reps, batch)
    s = r.ray_samples(rays, min_sigma=0.0, image_shape=shape)
    T = len(s)
    with torch.no_grad():
        w0, _ = svox.sample_weights(s, f[s.row.long(), -1].contiguous())
    w = w0.clone().requires_grad_(True)
    att = (1.0 - w0).clamp(0.0, 1.0).requires_grad_(True)         # factors in [0, 1], as attenuations are
    g = synth.grad_output(T, 1).cuda()[:, 0].contiguous()
    ray = s.ray.long()
    first = s.offsets[ray]                                        # every sample's first of its ray

    def hip_op(x, op):
        def step():
            x.grad = None
            svox.ray_scan(s, x, op).backward(g)
        return step

    def torch_sum():
        w.grad = None
        c = torch.cumsum(w, 0)
        before = (c - w)[first]                                   # the global sum in front of the ray
        (c - before).backward(g)

    t_sum, t_torch_sum = timed(hip_op(w, "sum"), reps, batch), timed(torch_sum, reps, batch)
    t_prod, t_max = timed(hip_op(att, "prod"), reps, batch), timed(hip_op(w, "max"), reps, batch)
    q3 = torch.tensor([0.25, 0.5, 0.75], device="cuda")
    t_quant = timed(lambda: svox.ray_quantile(s, w0, q3), reps, batch)

    keep = (torch.arange(T, device="cuda") * 2654435761 % 1000) < 500          # about half, scattered
    kept = int(keep.sum())

    def hip_select():
        s.select(keep)

    def torch_select(arrays):
        def step():
            index = torch.nonzero(keep)[:, 0]
            cols = [x.index_select(0, index) for x in arrays]
            counts = torch.zeros(Q, dtype=torch.int64, device=keep.device).index_add_(0, cols[0].long(), torch.ones_like(index))
            offsets = torch.zeros(Q + 1, dtype=torch.int64, device=keep.device)
            torch.cumsum(counts, 0, out=offsets[1:])
            return offsets, cols
        return step

    four = (s.ray, s.row, s.depth, s.length)                      # (the fifth: a per-sample tensor carried over, values[index])
    t_sel, t_torch_sel = timed(hip_select, reps, batch), timed(torch_select(four + (w0,)), reps, batch)
    t_torch_sel4 = timed(torch_select(four), reps, batch)
    ok_a, ok_b = t_sum <= t_torch_sum, t_sel <= t_torch_sel
    say(f"{name}: depth {depth}, K = {K}, {W} x {W} rays; {T} samples with sigma > 0, {T / Q:.1f} a ray, the longest list {int(s.counts.max())}")
    say(f"  (a) ray_scan(w, sum), fwd + bwd                       {t_sum:8.3f} ms")
    say(f"      cumsum - start value gathered through ray, fwd + bwd {t_torch_sum:8.3f} ms   HIP / PyTorch = {t_sum / t_torch_sum:.2f}   "
        f"gate (<= 1): {'holds' if ok_a else 'FAILS'}")
    say(f"  (b) select, {kept} of {T} kept                   {t_sel:8.3f} ms")
    say(f"      nonzero + 5 index_select + counts + cumsum          {t_torch_sel:8.3f} ms   HIP / PyTorch = {t_sel / t_torch_sel:.2f}   "
        f"gate (<= 1): {'holds' if ok_b else 'FAILS'}")
    say(f"      ... with 4 index_select (the lists alone)            {t_torch_sel4:8.3f} ms   HIP / PyTorch = {t_sel / t_torch_sel4:.2f}   (not gated)")
    say(f"  ray_scan(att, prod), fwd + bwd                        {t_prod:8.3f} ms   (not gated)")
    say(f"  ray_scan(w, max), fwd + bwd                           {t_max:8.3f} ms   (not gated)")
    say(f"  ray_quantile, nq = 3                                  {t_quant:8.3f} ms   (not gated)")
    say(f"  ray_samples(min_sigma = 0)                            {t_lists:8.3f} ms   select / ray_samples = {t_sel / t_lists:.2f}   (not gated)")
    return ok_a and ok_b


def one_workload(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("scan_timing: needs a GPU (a timing taken anywhere else says nothing)")
    print(f"scan_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}", flush=True)
    run("warm-up", 1, 1, lambda s: None)
    ok = run(args.only, args.reps, args.batch, lambda s: print(s, flush=True))
    sys.exit(0 if ok else GATE_FAILED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_timing.txt"))
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
            sys.exit(f"scan_timing: workload {name} ran into its limit of {LIMIT_S} s; nothing more is started")
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode not in (0, GATE_FAILED):
            sys.exit(f"scan_timing: workload {name} ended with status {res.returncode}; nothing more is started")
        ok = ok and res.returncode == 0
        out = res.stdout.splitlines()
        lines += out if not lines else out[1:]                    # the header once
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
