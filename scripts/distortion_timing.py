#!/usr/bin/env python3
"""render_distortion (csrc/svoxt_distort.hip) beside its sibling and the colour step, on the same GPU, tree and rays in
one process per workload, on the two benchmark workloads

    D8: the headline workload (synth depth 8, SH9, K = 28, 800 x 800)
    C4: the config-4 tree (synth depth 9, K = 32, 1024 x 1024)

per workload: render_distortion forward alone and forward + backward; render_depth_moments forward + backward (the same
march, records and table: the ratio is recorded, not gated); the colour step, VolumeRenderer.forward + backward.
GATE: render_distortion forward + backward must not take longer than the colour step -- the script exits with status 1
if it does.  Every figure is the median of `--reps` event timings of `--batch` steps each, taken after warm-up rounds
that go on until two consecutive rounds agree within 3 %.  Without --only every workload runs in a process of its own
and the lines are written to profiles/distortion_timing.txt.

    python scripts/distortion_timing.py [--reps 9] [--batch 10] [--only D8] [--samples 64]
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
    import svox_t_amd.csrc as _C
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
    g3 = synth.grad_output(Q, 3).cuda()
    g2 = synth.grad_output(Q, 2).cuda()
    with torch.no_grad():
        C1 = r(f, rays, image_shape=shape).shape[1]
    gc = synth.grad_output(Q, C1).cuda()

    def ds_fwd():
        with torch.no_grad():
            r.render_distortion(f, rays, image_shape=shape)

    def ds_step():
        f.grad = None
        r.render_distortion(f, rays, image_shape=shape).backward(g2)

    def dm_step():
        f.grad = None
        r.render_depth_moments(f, rays, at="mid", image_shape=shape).backward(g3)

    def colour_step():
        f.grad = None
        r(f, rays, image_shape=shape).backward(gc)

    t_f, t_ds, t_dm, t_col = (timed(fn, reps, batch) for fn in (ds_fwd, ds_step, dm_step, colour_step))
    # how many rays were longer than the lists (their tails are marched by the backward)
    ws_over = None
    spec = svox.renderer._rays_spec_from_rays(rays, shape)
    spec.need_grad = True
    _C.distortion(tree._spec(f), spec, r._get_options())
    plan = spec._svoxt_distortion_plan
    if plan is not None:
        qpad = (Q + 63) // 64 * 64
        aux = plan[2][:qpad * 8].view(torch.int32).view(qpad, 2)
        ws_over = int((aux[:, 0] < 0).sum())
    say(f"{name}: depth {depth}, K = {K}, {W} x {W} rays, M = {f.shape[0]} rows; lists of {_C._extras.DISTORTION_SAMPLES} "
        f"samples a ray, {ws_over} rays longer")
    say(f"  render_distortion forward                 {t_f:8.3f} ms")
    say(f"  render_distortion forward + backward      {t_ds:8.3f} ms")
    say(f"  render_depth_moments forward + backward   {t_dm:8.3f} ms   distortion / depth moments = {t_ds / t_dm:.2f}   (not gated)")
    say(f"  colour step (forward + backward)          {t_col:8.3f} ms   distortion / colour        = {t_ds / t_col:.2f}   "
        f"gate (<= 1): {'holds' if t_ds <= t_col else 'FAILS'}")
    return t_ds <= t_col


def one_workload(args):
    import torch
    import svox_t_amd.csrc as _C
    if not torch.cuda.is_available():
        sys.exit("distortion_timing: needs a GPU (a timing taken anywhere else says nothing)")
    if args.samples is not None:
        _C._extras.DISTORTION_SAMPLES = args.samples
        _C._extras.DEPTHMOM_SAMPLES = args.samples
    print(f"distortion_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}, thresholds 0", flush=True)
    run("warm-up", 1, 1, lambda s: None)
    ok = run(args.only, args.reps, args.batch, lambda s: print(s, flush=True))
    sys.exit(0 if ok else GATE_FAILED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--samples", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_timing.txt"))
    args = ap.parse_args()
    if args.only:
        one_workload(args)
    # one process per workload: this one never opens the GPU
    lines, ok = [], True
    for name in sorted(WORKLOADS, reverse=True):
        cmd = [sys.executable, os.path.abspath(__file__), "--only", name, "--reps", str(args.reps), "--batch", str(args.batch)]
        if args.samples is not None:
            cmd += ["--samples", str(args.samples)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode not in (0, GATE_FAILED):
            sys.exit(f"distortion_timing: workload {name} ended with status {res.returncode}")
        ok = ok and res.returncode == 0
        out = res.stdout.splitlines()
        lines += out if not lines else out[1:]                    # the header once
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
