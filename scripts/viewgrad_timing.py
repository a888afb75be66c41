#!/usr/bin/env python3
"""The gradient in the view direction (csrc/svoxt_shade.hip, DESIGN.md 4.30: view_basis in viewdirs, shade_samples in
basis) beside the route the package prescribed before it -- gather_rows over all K columns, the contraction and the
sigmoid as PyTorch ops, an SH9 basis written in torch, autograd to viewdirs -- on the same GPU, lists and tensors in one
process per workload, on the two benchmark geometries

    D8: the headline workload (synth depth 8, SH9, K = 28, 800 x 800)
    C4: the config-4 geometry (synth depth 9, 1024 x 1024) with SH9 rows of K = 28 -- its own rows are RGBA, K = 32, and
        have no basis to differentiate

per workload, on the lists of ray_samples(min_sigma = 0, faces = True), the feature table fixed (a pose is refined):
 (a) view_basis forward + backward to viewdirs beside the SH9 polynomials in torch with autograd.        GATE: HIP <= PyTorch
 (b) shade_samples forward + backward to basis beside gather_rows (all K columns) + contraction + sigmoid as PyTorch ops
     with autograd to the basis; peak bytes a sample above the inputs for both.                         GATE: HIP <= PyTorch
 (c) both together, viewdirs to colours and back: shade_samples(rays=) beside the whole composition.    GATE: HIP <= PyTorch
 not gated: shade_samples' backward to the feature table alone and with grad_basis as well; the colour chain --
     pinhole_rays(c2w) -> ray_samples(faces=True) -> sample_geometry + view_basis -> shade_samples -> sample_weights(length=)
     -> accumulate(colour), forward + backward to c2w.grad -- beside the depth chain of scripts/raygeom_timing.py.
The script exits with status 1 if a gate fails.  Every figure is the median of `--reps` event timings of `--batch` steps
each, taken after warm-up rounds that go on until two consecutive rounds agree within 3 %.  Without --only every workload
runs in a process of its own, under its own time limit, and the lines are written to profiles/viewgrad_timing.txt.

    python scripts/viewgrad_timing.py [--reps 9] [--batch 10] [--only D8]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"D8": (8, 800), "C4": (9, 1024)}
WARM_UP = (5, 64)
K, FMT, BD, C = 28, "SH9", 9, 3
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


def peak_bytes(fn):
    """The peak of allocated device memory above what is allocated before the call."""
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def torch_sh9(v):
    """The SH9 basis in PyTorch ops: the polynomials of the kernels without their bits."""
    import torch
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    return torch.stack([torch.full_like(x, 0.28209479177387814), -0.4886025119029199 * y, 0.4886025119029199 * z,
                        -0.4886025119029199 * x, 1.0925484305920792 * (x * y), -1.0925484305920792 * (y * z),
                        0.31539156525252005 * (2.0 * zz - xx - yy), -1.0925484305920792 * (x * z),
                        0.5462742152960396 * (xx - yy)], dim=1)


def run(name, reps, batch, say):
    import numpy as np
    import torch
    import svox_t_amd as svox
    from svox_t_amd import synth
    from svox_t_amd.renderer import pinhole_rays
    depth, W = WORKLOADS.get(name, WARM_UP)
    st = synth.shell_tree(depth)
    feats = synth.shell_features(st.n_features, K, seed=0)
    tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, data_format=FMT, device="cuda")
    r = svox.VolumeRenderer(tree)
    o, d, v = synth.pinhole_rays(W, W, c2w=synth.camera_pose())
    o, d, v = o.cuda(), d.cuda(), v.cuda()
    f = tree.features.detach()
    Q, shape = W * W, (W, W)
    s = r.ray_samples(svox.Rays(o, d, v), min_sigma=0.0, image_shape=shape, faces=True)
    T = len(s)
    ray = s.ray.long()
    g_values = synth.grad_output(T, C, seed=2).cuda()
    g_basis = synth.grad_output(Q, BD, seed=3).cuda()

    # (a) view_basis, forward + backward to viewdirs
    vv = v.clone().requires_grad_(True)

    def hip_view():
        vv.grad = None
        r.view_basis(svox.Rays(o, d, vv)).backward(g_basis)

    def torch_view():
        vv.grad = None
        torch_sh9(vv).backward(g_basis)

    t_view, t_view_torch = timed(hip_view, reps, batch), timed(torch_view, reps, batch)
    hip_view()
    a = vv.grad.clone()
    torch_view()
    apart_view = float((a - vv.grad).abs().max() / vv.grad.abs().max())

    # (b) shade_samples, forward + backward to basis
    basis = r.view_basis(svox.Rays(o, d, v)).requires_grad_(True)

    def torch_shade(b):
        rows = svox.gather_rows(s, f)                                           # [T, K]
        tmp = (rows[:, :C * BD].view(T, C, BD) * b[ray][:, None, :]).sum(-1)
        return torch.sigmoid(tmp)

    def hip_basis():
        basis.grad = None
        r.shade_samples(s, f, basis=basis)[0].backward(g_values)

    def torch_basis():
        basis.grad = None
        torch_shade(basis).backward(g_values)

    t_basis, t_basis_torch = timed(hip_basis, reps, batch), timed(torch_basis, reps, batch)
    m_basis, m_basis_torch = peak_bytes(hip_basis), peak_bytes(torch_basis)
    hip_basis()
    a = basis.grad.clone()
    torch_basis()
    apart_basis = float((a - basis.grad).abs().max() / basis.grad.abs().max())

    # (c) viewdirs -> colours -> viewdirs
    def hip_both():
        vv.grad = None
        r.shade_samples(s, f, svox.Rays(o, d, vv))[0].backward(g_values)

    def torch_both():
        vv.grad = None
        torch_shade(torch_sh9(vv)).backward(g_values)

    t_both, t_both_torch = timed(hip_both, reps, batch), timed(torch_both, reps, batch)
    m_both, m_both_torch = peak_bytes(hip_both), peak_bytes(torch_both)

    # not gated: the table's gradient alone and with grad_basis as well
    fg = f.clone().requires_grad_(True)
    s.row_plan(fg.shape[0])                                                     # (the plan is cached: not timed)
    b_plain = basis.detach()

    def bwd_table():
        fg.grad = None
        r.shade_samples(s, fg, basis=b_plain)[0].backward(g_values)

    def bwd_table_and_basis():
        fg.grad = basis.grad = None
        r.shade_samples(s, fg, basis=basis)[0].backward(g_values)

    t_table, t_table_basis = timed(bwd_table, reps, batch), timed(bwd_table_and_basis, reps, batch)

    # not gated: the colour chain beside the depth chain
    pose = torch.from_numpy(synth.camera_pose().astype(np.float32)).cuda()
    fx = 1111.111 * W / 800.0
    g3 = synth.grad_output(Q, C, seed=4).cuda()
    g1 = g3[:, 0].contiguous()
    sig_of = f[:, -1].contiguous()

    def chain(colour):
        c2w = pose.clone().requires_grad_(True)
        oo, dd, vd = pinhole_rays(c2w, W, W, fx, fx)
        rr = svox.Rays(oo, dd, vd)
        ss = r.ray_samples(rr, min_sigma=0.0, image_shape=shape, faces=True)
        z, ln = svox.sample_geometry(ss, rr)
        if colour:
            values, sigma = r.shade_samples(ss, f, rr)
            w, _ = svox.sample_weights(ss, sigma, length=ln)
            svox.accumulate(ss, w, values).backward(g3)
        else:
            w, _ = svox.sample_weights(ss, sig_of[ss.row.long()], length=ln)
            svox.accumulate(ss, w, z[:, None])[:, 0].backward(g1)
        return c2w.grad

    t_colour, t_depth = timed(lambda: chain(True), reps, batch), timed(lambda: chain(False), reps, batch)
    same = torch.equal(chain(True), chain(True))

    ok = [t_view <= t_view_torch, t_basis <= t_basis_torch, t_both <= t_both_torch]
    word = lambda x: "holds" if x else "FAILS"                                  # noqa: E731
    say(f"{name}: depth {depth}, SH9, K = {K}, {W} x {W} rays; {T} samples with sigma > 0, {T / Q:.1f} a ray, the longest list {int(s.counts.max())}")
    say(f"  (a) view_basis, fwd + bwd to viewdirs                              {t_view:8.3f} ms")
    say(f"      the SH9 polynomials in PyTorch ops, fwd + bwd                  {t_view_torch:8.3f} ms   HIP / PyTorch = {t_view / t_view_torch:.2f}   "
        f"gate (<= 1): {word(ok[0])}   (apart by {apart_view:.1e} of the largest entry)")
    say(f"  (b) shade_samples, fwd + bwd to basis                              {t_basis:8.3f} ms   peak {m_basis / T:6.1f} bytes a sample")
    say(f"      gather_rows (K columns) + contraction + sigmoid, fwd + bwd     {t_basis_torch:8.3f} ms   peak {m_basis_torch / T:6.1f} bytes a sample   "
        f"HIP / PyTorch = {t_basis / t_basis_torch:.2f}   gate (<= 1): {word(ok[1])}   (apart by {apart_basis:.1e}: the order of the atomics)")
    say(f"  (c) shade_samples(rays=), viewdirs -> colours -> viewdirs          {t_both:8.3f} ms   peak {m_both / T:6.1f} bytes a sample")
    say(f"      the whole composition in PyTorch ops                           {t_both_torch:8.3f} ms   peak {m_both_torch / T:6.1f} bytes a sample   "
        f"HIP / PyTorch = {t_both / t_both_torch:.2f}   gate (<= 1): {word(ok[2])}")
    say(f"  shade_samples fwd + bwd to the table / to the table and the basis  {t_table:8.3f} / {t_table_basis:8.3f} ms   (not gated)")
    say(f"  the colour chain c2w -> ... -> accumulate(colour), fwd + bwd       {t_colour:8.3f} ms   (c2w.grad twice the same bits: {same})")
    say(f"  the depth chain of raygeom_timing.py, fwd + bwd                    {t_depth:8.3f} ms   colour / depth = {t_colour / t_depth:.2f}   (not gated)")
    return all(ok)


def one_workload(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("viewgrad_timing: needs a GPU (a timing taken anywhere else says nothing)")
    print(f"viewgrad_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}", flush=True)
    run("warm-up", 1, 1, lambda s: None)
    ok = run(args.only, args.reps, args.batch, lambda s: print(s, flush=True))
    sys.exit(0 if ok else GATE_FAILED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viewgrad_timing.txt"))
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
            sys.exit(f"viewgrad_timing: workload {name} ran into its limit of {LIMIT_S} s; nothing more is started")
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode not in (0, GATE_FAILED):
            sys.exit(f"viewgrad_timing: workload {name} ended with status {res.returncode}; nothing more is started")
        ok = ok and res.returncode == 0
        out = res.stdout.splitlines()
        lines += out if not lines else out[1:]                    # the header once
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
