#!/usr/bin/env python3
"""The deterministic render backward (csrc/svoxt_rowgrad.hip; VolumeRenderer.forward(..., deterministic=True)) beside the
same gradient composed from the public per-sample operators, on the same GPU, tree, rays and upstream gradient in one
process per workload, on the two benchmark workloads

    D8: the headline workload (synth depth 8, SH9, K = 28, 800 x 800)
    C4: the config-4 tree (synth depth 9, K = 32, 1024 x 1024)

per workload, forward + backward of a fixed upstream gradient:
  fused     renderer(features, rays, deterministic=True).backward(g)
  composed  ray_samples(min_sigma = 0) -> gather_rows over all K columns -> shading in torch ops (the SH basis per ray,
            or the RGBA sigmoid) -> sample_weights -> accumulate(C) plus the background term -> .backward(g)
            GATE: the fused form must not take longer than the composed form -- the script exits with status 1 if it does;
recorded beside them, not gated:
  atomic    the default step, renderer(features, rays).backward(g), and the ratio fused / atomic;
  the split of the fused backward into its steps (count, record march, plan build, shade + per-ray passes with the plan's
  host read, row reduction), by events around them;
  the bytes of its workspace per sample.
Every figure is the median of `--reps` event timings of `--batch` steps each, taken after warm-up rounds that go on until
two consecutive rounds agree within 3 %.  Without --only every workload runs in a process of its own and the lines are
written to profiles/rowgrad_timing.txt.

    python scripts/rowgrad_timing.py [--reps 9] [--batch 10] [--only D8]
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
STEPS = ("count", "emit", "plan", "sweep", "reduce")        # the march twice, the plan build, shade + per-ray passes, the rows


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


def sh9_basis(d):
    """[Q, 9] real spherical harmonics of degree <= 2 at unit directions d [Q, 3], in torch ops: the reference's
    sh.eval_sh_bases(2, d) (svox_t/sh.py:114-162), which this package does not carry as a module of its own."""
    import torch
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return torch.stack([torch.full_like(x, 0.28209479177387814), -0.4886025119029199 * y, 0.4886025119029199 * z,
                        -0.4886025119029199 * x, 1.0925484305920792 * x * y, -1.0925484305920792 * y * z,
                        0.31539156525252005 * (2.0 * z * z - x * x - y * y), -1.0925484305920792 * x * z,
                        0.5462742152960396 * (x * x - y * y)], dim=1)


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
    table = tree.features.detach().clone().requires_grad_(True)
    M, Q = table.shape[0], W * W
    sh = fmt != "RGBA"
    C = 3 if sh else K - 1
    g = synth.grad_output(Q, C + 1).cuda()
    bg = float(r.background_brightness)

    def fused():
        table.grad = None
        r(table, rays, deterministic=True, image_shape=(W, W)).backward(g)

    def atomic():
        table.grad = None
        r(table, rays, image_shape=(W, W)).backward(g)

    def composed():
        table.grad = None
        s = r.ray_samples(rays, min_sigma=0.0, image_shape=(W, W))
        rows = svox.gather_rows(s, table)
        if sh:
            basis = sh9_basis(rays.viewdirs)[s.ray.long()]
            colour = torch.sigmoid((rows[:, :-1].view(-1, C, 9) * basis[:, None, :]).sum(-1))
        else:
            colour = torch.sigmoid(rows[:, :-1])
        w, alpha = svox.sample_weights(s, rows[:, -1].contiguous())
        out = svox.accumulate(s, w, colour.contiguous()) + bg * (1.0 - alpha)[:, None]
        torch.cat([out, alpha[:, None]], dim=1).backward(g)

    # the two are the same gradient: a look before the clocks start
    fused()
    g_fused = table.grad.clone()
    composed()
    scale = g_fused.abs().max().item()
    apart = (table.grad - g_fused).abs().max().item() / max(scale, 1e-30)
    if not apart <= 1e-5:                       # (float32 sums in two orders: 1e-7; anything else is another gradient)
        sys.exit(f"rowgrad_timing: the fused and the composed gradient are {apart:.1e} of the largest entry apart")
    t_fused, t_comp, t_atomic = timed(fused, reps, batch), timed(composed, reps, batch), timed(atomic, reps, batch)
    ok = t_fused <= t_comp

    # the split of the backward alone, by events around its steps
    spec, rspec, opt = r.tree._spec(table.detach()), svox.renderer._rays_spec_from_rays(rays, (W, W)), r._get_options()
    split = {k: [] for k in STEPS}
    for _ in range(max(reps, 3) + 2):
        marks = []

        def tick(step):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((step, e))

        _C.volume_render_backward_rows(spec, rspec, opt, g, timers=tick)
        torch.cuda.synchronize()
        for (step, a), (_, b) in zip(marks, marks[1:]):
            split[step].append(a.elapsed_time(b))
    med = {k: sorted(x[2:])[len(x[2:]) // 2] for k, x in split.items()}         # (the first two rounds warm up)
    last = _C._extras.ROWGRAD_LAST
    T = last["T"]
    plan_ws = _C._lib.svoxt_row_plan_workspace_bytes(T, M)
    say(f"{name}: depth {depth}, K = {K}, {W} x {W} rays, M = {M} rows; {T} samples with sigma > 0, the longest row {last['longest']}, "
        f"{last['n_long']} rows of more than 256")
    say(f"  fused     forward(deterministic=True) + backward        {t_fused:8.3f} ms")
    say(f"  composed  ray_samples .. accumulate in torch + backward {t_comp:8.3f} ms   fused / composed = {t_fused / t_comp:.2f}   "
        f"gate (<= 1): {'holds' if ok else 'FAILS'}   (max |difference| of the two gradients / max |gradient| = {apart:.1e})")
    say(f"  atomic    forward() + backward, the default             {t_atomic:8.3f} ms   fused / atomic = {t_fused / t_atomic:.2f}   (not gated)")
    say("  the deterministic backward alone: " + ", ".join(f"{k} {med[k]:.3f}" for k in STEPS) + f" ms (sum {sum(med.values()):.3f})")
    say(f"  its workspace: {last['bytes']} bytes = {last['bytes'] / max(T, 1):.1f} a sample, of which the row plan's own sort "
        f"workspace {plan_ws / max(T, 1):.1f}; the bound 4 (C + 4) + 4 (perm) = {4 * (C + 4) + 4}")
    return ok


def one_workload(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("rowgrad_timing: needs a GPU (a timing taken anywhere else says nothing)")
    print(f"rowgrad_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}", flush=True)
    run("warm-up", 1, 1, lambda s: None)
    ok = run(args.only, args.reps, args.batch, lambda s: print(s, flush=True))
    sys.exit(0 if ok else GATE_FAILED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rowgrad_timing.txt"))
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
            sys.exit(f"rowgrad_timing: workload {name} ended with status {res.returncode}")
        ok = ok and res.returncode == 0
        out = res.stdout.splitlines()
        lines += out if not lines else out[1:]                    # the header once
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
