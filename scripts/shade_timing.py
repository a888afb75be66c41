#!/usr/bin/env python3
"""shade_samples (csrc/svoxt_shade.hip) beside the composition it replaces, on the same GPU, tree, rays and lists in one
process per workload, on the two benchmark workloads

    D8: the headline workload (synth depth 8, SH9, K = 28, 800 x 800)
    C4: the config-4 tree (synth depth 9, K = 32, 1024 x 1024)

per workload, on the lists of ray_samples(min_sigma = 0), with a warm row plan and the rays' basis from view_basis,
forward + backward of fixed upstream gradients (g_values [T, C], g_sigma [T]):
  HIP       renderer.shade_samples(samples, table, basis=basis), then backward
  composed  gather_rows over all K columns -> the basis contraction and the sigmoid as torch ops (RGBA: the sigmoid) ->
            backward, on the same tensors
            GATE: the HIP form must not take longer than the composed form -- the script exits with status 1 if it does;
recorded beside them, not gated:
  the peak of torch.cuda.max_memory_allocated over one step of either form, above what is allocated before it;
  the forward alone (rowgrad_timing's sweep holds the same shade: profiles/rowgrad_timing.txt), view_basis alone, and for
  RGBA rows the forward over the same table one float further on (the scalar kernel instead of the 16-byte one).
Every figure is the median of `--reps` event timings of `--batch` steps each, taken after warm-up rounds that go on until
two consecutive rounds agree within 3 %.  Without --only every workload runs in a process of its own and the lines are
written to profiles/shade_timing.txt.

    python scripts/shade_timing.py [--reps 9] [--batch 10] [--only D8]
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


def peak_of(fn):
    """Bytes one call of fn allocates at its peak, above what is allocated when it starts."""
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


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
    s = r.ray_samples(rays, min_sigma=0.0, image_shape=(W, W))
    T, M = len(s), tree.features.shape[0]
    table = tree.features.detach().clone().requires_grad_(True)
    sh = fmt != "RGBA"
    bd = r.data_format.basis_dim if sh else 0
    C = (K - 1) // bd if sh else K - 1
    basis = r.view_basis(rays)
    gv, gs = synth.grad_output(T, C).cuda(), synth.grad_output(T, 1, seed=2).cuda()[:, 0].contiguous()
    ray_l = s.ray.long()
    s.row_plan(M)

    def hip():
        table.grad = None
        values, sigma = r.shade_samples(s, table, basis=basis)
        torch.autograd.backward([values, sigma], [gv, gs])

    def composed():
        table.grad = None
        rows = svox.gather_rows(s, table)
        if sh:
            colour = torch.sigmoid((rows[:, :C * bd].view(-1, C, bd) * basis[ray_l][:, None, :]).sum(-1))
        else:
            colour = torch.sigmoid(rows[:, :-1])
        torch.autograd.backward([colour, rows[:, -1]], [gv, gs])

    hip()
    g_hip = table.grad.clone()
    composed()
    diff = float((table.grad - g_hip).abs().max() / g_hip.abs().max())
    t_hip, t_comp = timed(hip, reps, batch), timed(composed, reps, batch)
    ok = t_hip <= t_comp
    p_hip, p_comp = peak_of(hip), peak_of(composed)

    with torch.no_grad():
        plain = table.detach()
        t_fwd = timed(lambda: r.shade_samples(s, plain, basis=basis), reps, batch)
        t_basis = timed(lambda: r.view_basis(rays), reps, batch)
        t_scalar = None
        if not sh and K % 4 == 0:
            shifted = torch.empty(M * K + 1, device="cuda")[1:].view(M, K)
            shifted.copy_(plain)
            t_scalar = timed(lambda: r.shade_samples(s, shifted), reps, batch)

    plan = s.row_plan(M)
    say(f"{name}: depth {depth}, K = {K}, C = {C}, {W} x {W} rays, M = {M} rows; {T} samples with sigma > 0, the longest row "
        f"{plan.longest}, {plan.long_rows.shape[0]} rows of more than 256")
    say(f"  HIP       shade_samples, fwd + bwd                         {t_hip:8.3f} ms")
    say(f"  composed  gather_rows (all {K} columns) + torch ops, fwd + bwd {t_comp:8.3f} ms   HIP / composed = {t_hip / t_comp:.2f}   "
        f"gate (<= 1): {'holds' if ok else 'FAILS'}   (max |difference| of the two gradients / max |gradient| = {diff:.1e})")
    say(f"  peak bytes of one step above the inputs: HIP {p_hip} = {p_hip / T:.1f} a sample, composed {p_comp} = {p_comp / T:.1f} "
        f"a sample; the outputs alone 4 (C + 1) = {4 * (C + 1)}, a [T, K] tensor 4 K = {4 * K}   (not gated)")
    say(f"  the forward alone {t_fwd:8.3f} ms; view_basis ({W * W} rays) {t_basis:8.3f} ms"
        + ("" if t_scalar is None else f"; the forward over a table that is not 16-byte aligned (the scalar kernel) {t_scalar:8.3f} ms")
        + "   (not gated)")
    return ok


def one_workload(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("shade_timing: needs a GPU (a timing taken anywhere else says nothing)")
    print(f"shade_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}", flush=True)
    run("warm-up", 1, 1, lambda s: None)
    ok = run(args.only, args.reps, args.batch, lambda s: print(s, flush=True))
    sys.exit(0 if ok else GATE_FAILED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_timing.txt"))
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
            sys.exit(f"shade_timing: workload {name} ended with status {res.returncode}")
        ok = ok and res.returncode == 0
        out = res.stdout.splitlines()
        lines += out if not lines else out[1:]                    # the header once
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
