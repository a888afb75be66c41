#!/usr/bin/env python3
"""render_depth_moments (csrc/svoxt_depthmom.hip) beside the two operators that run the same march, on the same GPU in
one process, on the two benchmark workloads

    D8: the headline workload (synth depth 8, SH9, K = 28, 800 x 800)
    C4: the config-4 tree (synth depth 9, K = 32, 1024 x 1024)

per workload: render_depth_moments forward alone and forward + backward; opacity_render forward + backward (the same
march, a gradient of the same shape: the floor); the colour step, VolumeRenderer.forward + backward (a superset of the
work).  GATE: render_depth_moments forward + backward must not take longer than the colour step -- the script exits
with status 1 if it does.  Every figure is the median of `--reps` event timings of `--batch` steps each, taken after
warm-up rounds that go on until two consecutive rounds agree within 3 %.  Writes profiles/depth_moments_timing.txt.

    python scripts/depth_moments_timing.py [--reps 9] [--batch 10] [--only D8] [--samples 64]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import svox_t_amd as svox                      # noqa: E402
import svox_t_amd.csrc as _C                   # noqa: E402
from svox_t_amd import synth                   # noqa: E402

WORKLOADS = {"D8": (8, 28, "SH9", 800), "C4": (9, 32, "RGBA", 1024)}
WARM_UP = (5, 28, "SH9", 64)


def round_of(fn, batch):
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
    g1 = synth.grad_output(Q, 1).cuda()
    with torch.no_grad():
        C1 = r(f, rays, image_shape=shape).shape[1]
    gc = synth.grad_output(Q, C1).cuda()

    def dm_fwd():
        with torch.no_grad():
            r.render_depth_moments(f, rays, image_shape=shape)

    def dm_step():
        f.grad = None
        r.render_depth_moments(f, rays, image_shape=shape).backward(g3)

    def op_step():
        f.grad = None
        r.opacity_render(f, rays, image_shape=shape).backward(g1)

    def colour_step():
        f.grad = None
        r(f, rays, image_shape=shape).backward(gc)

    t_f, t_dm, t_op, t_col = (timed(fn, reps, batch) for fn in (dm_fwd, dm_step, op_step, colour_step))
    # how many rays were longer than the lists (their tails are marched by the backward)
    ws_over = None
    spec = svox.renderer._rays_spec_from_rays(rays, shape)
    spec.need_grad = True
    _C.depth_moments(tree._spec(f), spec, r._get_options())
    plan = spec._svoxt_depth_plan
    if plan is not None:
        qpad = (Q + 63) // 64 * 64
        aux = plan[2][:qpad * 8].view(torch.int32).view(qpad, 2)
        ws_over = int((aux[:, 0] < 0).sum())
    say(f"{name}: depth {depth}, K = {K}, {W} x {W} rays, M = {f.shape[0]} rows; lists of {_C._extras.DEPTHMOM_SAMPLES} samples a ray, "
        f"{ws_over} rays longer")
    say(f"  render_depth_moments forward            {t_f:8.3f} ms")
    say(f"  render_depth_moments forward + backward {t_dm:8.3f} ms")
    say(f"  opacity_render forward + backward       {t_op:8.3f} ms   depth moments / opacity = {t_dm / t_op:.2f}")
    say(f"  colour step (forward + backward)        {t_col:8.3f} ms   depth moments / colour  = {t_dm / t_col:.2f}   "
        f"gate (<= 1): {'holds' if t_dm <= t_col else 'FAILS'}")
    del tree
    return t_dm <= t_col


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--samples", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_moments_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("depth_moments_timing: needs a GPU (a timing taken anywhere else says nothing)")
    if args.samples is not None:
        _C._extras.DEPTHMOM_SAMPLES = args.samples
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"depth_moments_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}, at = entry, thresholds 0")
    run("warm-up", 1, 1, lambda s: None)
    ok = True
    for name in ([args.only] if args.only else sorted(WORKLOADS, reverse=True)):
        ok = run(name, args.reps, args.batch, say) and ok
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
