#!/usr/bin/env python3
"""shade_samples(rotations=) (csrc/svoxt_viewrot.hip) beside the only route a user had before it -- the
same computation as PyTorch ops with autograd: rotations[row] and viewdirs[ray] gathered, their product, an SH9 basis
written in torch, gather_rows over all K columns, the contraction and the sigmoid -- on the same GPU, lists and tensors in
one process per workload, on the two benchmark geometries

    D8: the headline workload (synth depth 8, SH9, K = 28, 800 x 800)
    C4: the config-4 geometry (synth depth 9, 1024 x 1024) with SH9 rows of K = 28 -- its own rows are RGBA, K = 32, and
        have no basis to rotate

per workload, on the lists of ray_samples(min_sigma = 0), with general [M, 3, 3] matrices:
 (a) forward + backward with `features` alone requiring grad.                                    GATE: HIP <= PyTorch
 (b) forward + backward with features, rotations and viewdirs requiring grad.                    GATE: HIP <= PyTorch
     peak bytes a sample above the inputs, for (a) and (b).                                      GATE: HIP < PyTorch
 not gated: the forward alone; the cost over the unrotated shade_samples step (forward + backward to the table).
The script exits with status 1 if a gate fails.  Every figure is the median of `--reps` event timings of `--batch` steps
each, taken after warm-up rounds that go on until two consecutive rounds agree within 3 %.  Without --only every workload
runs in a process of its own, under its own time limit, and the lines are written to profiles/viewrot_timing.txt.

    python scripts/viewrot_timing.py [--reps 9] [--batch 10] [--only D8]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from viewgrad_timing import peak_bytes, timed, torch_sh9  # noqa: E402  (the family's timing rule and the SH9 polynomials)

WORKLOADS = {"D8": (8, 800), "C4": (9, 1024)}
WARM_UP = (5, 64)
K, FMT, BD, C = 28, "SH9", 9, 3
GATE_FAILED = 3
LIMIT_S = 400                                   # a workload's process


def run(name, reps, batch, say):
    import torch
    import svox_t_amd as svox
    from svox_t_amd import synth
    depth, W = WORKLOADS.get(name, WARM_UP)
    st = synth.shell_tree(depth)
    feats = synth.shell_features(st.n_features, K, seed=0)
    tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, data_format=FMT, device="cuda")
    r = svox.VolumeRenderer(tree)
    o, d, v = synth.pinhole_rays(W, W, c2w=synth.camera_pose())
    o, d, v = o.cuda(), d.cuda(), v.cuda()
    f0 = tree.features.detach()
    M, Q, shape = f0.shape[0], W * W, (W, W)
    s = r.ray_samples(svox.Rays(o, d, v), min_sigma=0.0, image_shape=shape)
    T = len(s)
    row, ray = s.row.long(), s.ray.long()
    g_values = synth.grad_output(T, C, seed=2).cuda()
    gen = torch.Generator().manual_seed(5)
    rot0 = (torch.eye(3)[None] + 0.2 * torch.randn(M, 3, 3, generator=gen)).cuda()
    s.row_plan(M)                                                               # (the plan is cached: not timed)

    def leaves(all_three):
        return f0.clone().requires_grad_(True), rot0.clone().requires_grad_(all_three), v.clone().requires_grad_(all_three)

    def hip_step(f, R, vv):
        f.grad = R.grad = vv.grad = None
        r.shade_samples(s, f, svox.Rays(o, d, vv), rotations=R)[0].backward(g_values)

    def torch_step(f, R, vv):
        f.grad = R.grad = vv.grad = None
        u = (R[row] * vv[ray][:, None, :]).sum(-1)                              # [T, 3]: the rotated directions
        rows = svox.gather_rows(s, f)                                           # [T, K]
        tmp = (rows[:, :C * BD].view(T, C, BD) * torch_sh9(u)[:, None, :]).sum(-1)
        torch.sigmoid(tmp).backward(g_values)

    res = {}
    for key, all_three in (("a", False), ("b", True)):
        x = leaves(all_three)
        t_hip, t_torch = timed(lambda: hip_step(*x), reps, batch), timed(lambda: torch_step(*x), reps, batch)
        m_hip, m_torch = peak_bytes(lambda: hip_step(*x)), peak_bytes(lambda: torch_step(*x))
        hip_step(*x)
        mine = [t.grad.clone() for t in x if t.grad is not None]
        torch_step(*x)
        theirs = [t.grad for t in x if t.grad is not None]
        apart = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(mine, theirs))
        res[key] = (t_hip, t_torch, m_hip, m_torch, apart)
        del x, mine, theirs
        torch.cuda.empty_cache()

    vv = v.clone()

    def fwd_rot():
        with torch.no_grad():
            r.shade_samples(s, f0, svox.Rays(o, d, vv), rotations=rot0)

    def fwd_plain():
        with torch.no_grad():
            r.shade_samples(s, f0, svox.Rays(o, d, vv))

    fg = f0.clone().requires_grad_(True)

    def plain_step():
        fg.grad = None
        r.shade_samples(s, fg, svox.Rays(o, d, vv))[0].backward(g_values)

    t_fwd, t_fwd_plain, t_plain = timed(fwd_rot, reps, batch), timed(fwd_plain, reps, batch), timed(plain_step, reps, batch)

    ok = [res["a"][0] <= res["a"][1], res["b"][0] <= res["b"][1], res["a"][2] < res["a"][3], res["b"][2] < res["b"][3]]
    word = lambda x: "holds" if x else "FAILS"                                  # noqa: E731
    say(f"{name}: depth {depth}, SH9, K = {K}, {W} x {W} rays, {M} feature rows; {T} samples with sigma > 0, {T / Q:.1f} a ray, "
        f"the longest row {s.row_plan(M).longest}")
    for key, what, i in (("a", "features alone require grad", 0), ("b", "features, rotations and viewdirs require grad", 1)):
        t_hip, t_torch, m_hip, m_torch, apart = res[key]
        say(f"  ({key}) shade_samples(rotations=), fwd + bwd, {what:<46} {t_hip:8.3f} ms   peak {m_hip / T:6.1f} bytes a sample")
        say(f"      the same computation in PyTorch ops with autograd                  {'':<20} {t_torch:8.3f} ms   peak {m_torch / T:6.1f} bytes a sample   "
            f"HIP / PyTorch = {t_hip / t_torch:.2f}   gate (<= 1): {word(ok[i])}   bytes gate (<): {word(ok[2 + i])}   (apart by {apart:.1e} of the largest entry)")
    say(f"  the forward alone, rotated / unrotated                                  {t_fwd:8.3f} / {t_fwd_plain:8.3f} ms   (not gated)")
    say(f"  the unrotated shade_samples step, fwd + bwd to the table                {t_plain:8.3f} ms   rotated (a) / unrotated = "
        f"{res['a'][0] / t_plain:.2f}   (not gated)")
    return all(ok)


def one_workload(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("viewrot_timing: needs a GPU (a timing taken anywhere else says nothing)")
    print(f"viewrot_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}", flush=True)
    run("warm-up", 1, 1, lambda s: None)
    ok = run(args.only, args.reps, args.batch, lambda s: print(s, flush=True))
    sys.exit(0 if ok else GATE_FAILED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viewrot_timing.txt"))
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
            sys.exit(f"viewrot_timing: workload {name} ran into its limit of {LIMIT_S} s; nothing more is started")
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode not in (0, GATE_FAILED):
            sys.exit(f"viewrot_timing: workload {name} ended with status {res.returncode}; nothing more is started")
        ok = ok and res.returncode == 0
        out = res.stdout.splitlines()
        lines += out if not lines else out[1:]                    # the header once
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
