#!/usr/bin/env python3
"""se_grad (csrc/svoxt_rowgrad.hip, svoxt_render_hess_rows_*; VolumeRenderer.se_grad) beside the step it extends, on the
same GPU, tree, rays and target colours in one process per workload, on the two benchmark workloads

    D8: the headline workload (synth depth 8, SH9, K = 28, 800 x 800)
    C4: the config-4 tree (synth depth 9, K = 32, 1024 x 1024)

per workload:
  se_grad   renderer.se_grad(features, rays, colors): out + loss + grad + hessdiag
  step      renderer(features, rays, deterministic=True) -> torch MSE against the same colours -> .backward(): out + loss
            + grad, the code as it was before se_grad
            GATE: se_grad must not take longer than 2 x step -- a second full run of the pipeline over squared values would
            cost exactly two steps; the script exits with status 1 if the gate fails;
recorded beside them, not gated:
  the split of volume_render_hess_rows into its steps (count, record march, plan build, shade + per-ray passes with the
  plan's host read, the two row reductions), by events around them, beside volume_render_backward_rows' split;
  the bytes of its workspace per sample;
  gauss_newton_step_ beside the same three torch ops.
Every figure is the median of `--reps` event timings of `--batch` steps each, taken after warm-up rounds that go on until
two consecutive rounds agree within 3 %.  Without --only every workload runs in a process of its own and the lines are
written to profiles/segrad_timing.txt.

    python scripts/segrad_timing.py [--reps 9] [--batch 10] [--only D8]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.rowgrad_timing import GATE_FAILED, STEPS, WARM_UP, WORKLOADS, timed  # noqa: E402


def split_of(call, reps):
    """{step: median ms} of a call that takes timers=, by events around its steps (the first two rounds warm up)."""
    import torch
    split = {k: [] for k in STEPS}
    for _ in range(max(reps, 3) + 2):
        marks = []

        def tick(step):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((step, e))

        call(tick)
        torch.cuda.synchronize()
        for (step, a), (_, b) in zip(marks, marks[1:]):
            split[step].append(a.elapsed_time(b))
    return {k: sorted(x[2:])[len(x[2:]) // 2] for k, x in split.items()}


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
    C = 3 if fmt != "RGBA" else K - 1
    colors = torch.rand(Q, C, generator=torch.Generator().manual_seed(1)).cuda()

    def se_grad():
        return r.se_grad(table, rays, colors, image_shape=(W, W))

    def step():
        table.grad = None
        out = r(table, rays, deterministic=True, image_shape=(W, W))
        loss = ((out[:, :C] - colors) ** 2).mean()
        loss.backward()
        return loss

    # the two give the same gradient: a look before the clocks start
    res = se_grad()
    step()
    apart = (res.grad - table.grad).abs().max().item() / max(table.grad.abs().max().item(), 1e-30)
    if not apart <= 1e-6:                       # (autograd may round the residual's coefficient another way: 1e-7)
        sys.exit(f"segrad_timing: se_grad's gradient and the step's are {apart:.1e} of the largest entry apart")
    t_se, t_step = timed(se_grad, reps, batch), timed(step, reps, batch)
    ok = t_se <= 2.0 * t_step

    spec, rspec, opt = r.tree._spec(table.detach()), svox.renderer._rays_spec_from_rays(rays, (W, W)), r._get_options()
    g = torch.zeros(Q, C + 1, device="cuda")
    g[:, :C] = (res.out[:, :C] - colors) * (2.0 / colors.numel())
    curv = torch.zeros_like(g)
    curv[:, :C] = 2.0 / colors.numel()
    med_h = split_of(lambda tick: _C._extras.volume_render_hess_rows(spec, rspec, opt, g, curv, timers=tick), reps)
    med_g = split_of(lambda tick: _C.volume_render_backward_rows(spec, rspec, opt, g, timers=tick), reps)
    last, last_g = _C._extras.ROWHESS_LAST, _C._extras.ROWGRAD_LAST
    T = last["T"]

    p = table.detach().clone()
    grad, hess = res.grad, res.hessdiag

    def newton():
        svox.gauss_newton_step_(p, grad, hess, lr=1.0, damping=1e-4)

    def newton_torch():
        dd = hess + 1e-4
        p.copy_(torch.where(dd > 0, p - 1.0 * (grad / dd), p))

    t_gn, t_gn_torch = timed(newton, reps, batch), timed(newton_torch, reps, batch)

    say(f"{name}: depth {depth}, K = {K}, {W} x {W} rays, M = {M} rows; {T} samples with sigma > 0, the longest row {last['longest']}, "
        f"{last['n_long']} rows of more than 256")
    say(f"  se_grad   out + loss + grad + hessdiag                               {t_se:8.3f} ms")
    say(f"  step      forward(deterministic=True) + torch MSE + backward()       {t_step:8.3f} ms   se_grad / step = {t_se / t_step:.2f}   "
        f"gate (<= 2): {'holds' if ok else 'FAILS'}   (max |difference| of the two gradients / max |gradient| = {apart:.1e})")
    say("  volume_render_hess_rows alone:     " + ", ".join(f"{k} {med_h[k]:.3f}" for k in STEPS) + f" ms (sum {sum(med_h.values()):.3f})")
    say("  volume_render_backward_rows alone: " + ", ".join(f"{k} {med_g[k]:.3f}" for k in STEPS) + f" ms (sum {sum(med_g.values()):.3f})")
    say(f"  workspace: {last['bytes']} bytes = {last['bytes'] / max(T, 1):.1f} a sample (the gradient's: {last_g['bytes'] / max(T, 1):.1f}); "
        f"persistent 4 (C + 5) + 4 (perm) = {4 * (C + 5) + 4}, the transient [T, C] {4 * C}")
    say(f"  gauss_newton_step_ {t_gn:.3f} ms, the three torch ops (+ where, copy_) {t_gn_torch:.3f} ms over {M} x {K}")
    return ok


def one_workload(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("segrad_timing: needs a GPU (a timing taken anywhere else says nothing)")
    print(f"segrad_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}", flush=True)
    run("warm-up", 1, 1, lambda s: None)
    ok = run(args.only, args.reps, args.batch, lambda s: print(s, flush=True))
    sys.exit(0 if ok else GATE_FAILED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segrad_timing.txt"))
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
            sys.exit(f"segrad_timing: workload {name} ended with status {res.returncode}")
        ok = ok and res.returncode == 0
        out = res.stdout.splitlines()
        lines += out if not lines else out[1:]                    # the header once
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
