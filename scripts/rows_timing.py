#!/usr/bin/env python3
"""Samples to feature rows and back (csrc/svoxt_rows.hip) beside the torch indexing it replaces, on the same GPU, tree,
rays and lists in one process per workload, on the two benchmark workloads

    D8: the headline workload (synth depth 8, SH9, K = 28, 800 x 800)
    C4: the config-4 tree (synth depth 9, K = 32, 1024 x 1024)

per workload, on the lists of ray_samples(min_sigma = 0), with a warm row plan:
 (i)  gather_rows over all K columns, forward + backward of a fixed upstream gradient, beside table[row.long()] with
      autograd on the same tensors;
 (ii) reduce_rows(w, "max") beside torch.zeros(M).index_reduce_(0, row.long(), w, "amax").
      GATE, for both: the HIP form must not take longer than the PyTorch form -- the script exits with status 1 if it does;
recorded beside them, not gated:
      the plan build (sort, row_ptr, marks, one host read, the long-row lists) next to torch.sort(row, stable=True);
      on D8, (i) with the lists folded onto 4096 rows (row % 4096: about 1400 samples a row, the palette case).
Every figure is the median of `--reps` event timings of `--batch` steps each, taken after warm-up rounds that go on until
two consecutive rounds agree within 3 %.  Without --only every workload runs in a process of its own and the lines are
written to profiles/rows_timing.txt.

    python scripts/rows_timing.py [--reps 9] [--batch 10] [--only D8]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"D8": (8, 28, "SH9", 800), "C4": (9, 32, "RGBA", 1024)}
WARM_UP = (5, 28, "SH9", 64)
FOLD = 4096
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


def gather_pair(svox, s, table, g, reps, batch):
    """(HIP ms, PyTorch ms) of the gather over all columns, forward + backward of g, with a warm plan."""
    rowl = s.row.long()
    s.row_plan(table.shape[0])

    def hip():
        table.grad = None
        svox.gather_rows(s, table).backward(g)

    def torch_form():
        table.grad = None
        table[rowl].backward(g)

    return timed(hip, reps, batch), timed(torch_form, reps, batch)


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
    T, M = len(s), tree.features.shape[0]
    table = tree.features.detach().clone().requires_grad_(True)
    g = synth.grad_output(T, K).cuda()
    rowl = s.row.long()

    t_hip, t_torch = gather_pair(svox, s, table, g, reps, batch)
    ok = t_hip <= t_torch

    with torch.no_grad():
        w, _ = svox.sample_weights(s, table.detach()[rowl, -1].contiguous())

        def hip_max():
            svox.reduce_rows(s, w, M, "max")

        def torch_max():
            torch.zeros(M, device=w.device).index_reduce_(0, rowl, w, "amax")

        t_rmax, t_tmax = timed(hip_max, reps, batch), timed(torch_max, reps, batch)
        ok_max = t_rmax <= t_tmax

        def plan_build():
            _C.row_plan(s.row, M)

        def torch_sort():
            torch.sort(s.row, stable=True)

        t_plan, t_sort = timed(plan_build, reps, batch), timed(torch_sort, reps, batch)
    plan = s.row_plan(M)
    say(f"{name}: depth {depth}, K = {K}, {W} x {W} rays, M = {M} rows; {T} samples with sigma > 0, the longest segment "
        f"{plan.longest}, {plan.long_rows.shape[0]} rows of more than 256")
    say(f"  (i)  gather_rows, all {K} columns, fwd + bwd           {t_hip:8.3f} ms")
    say(f"       table[row.long()], fwd + bwd                     {t_torch:8.3f} ms   HIP / PyTorch = {t_hip / t_torch:.2f}   "
        f"gate (<= 1): {'holds' if ok else 'FAILS'}")
    say(f"  (ii) reduce_rows(w, \"max\")                             {t_rmax:8.3f} ms")
    say(f"       zeros(M).index_reduce_(0, row, w, \"amax\")         {t_tmax:8.3f} ms   HIP / PyTorch = {t_rmax / t_tmax:.2f}   "
        f"gate (<= 1): {'holds' if ok_max else 'FAILS'}")
    say(f"  the plan build, one host read                         {t_plan:8.3f} ms")
    say(f"       torch.sort(row, stable=True)                     {t_sort:8.3f} ms   plan / sort = {t_plan / t_sort:.2f}   (not gated)")
    if name == "D8":
        folded = svox.RaySamples(s.offsets, s.ray, (s.row % FOLD).contiguous(), s.depth, s.length)
        palette = table.detach()[:FOLD].clone().requires_grad_(True)
        f_hip, f_torch = gather_pair(svox, folded, palette, g, reps, batch)
        fp = folded.row_plan(FOLD)
        say(f"  (i) folded onto {FOLD} rows (the longest segment {fp.longest}, {fp.chunk_long.shape[0]} chunks), fwd + bwd")
        say(f"       gather_rows                                      {f_hip:8.3f} ms")
        say(f"       table[row.long()]                                {f_torch:8.3f} ms   HIP / PyTorch = {f_hip / f_torch:.2f}   (not gated)")
    return ok and ok_max


def one_workload(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("rows_timing: needs a GPU (a timing taken anywhere else says nothing)")
    print(f"rows_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}", flush=True)
    run("warm-up", 1, 1, lambda s: None)
    ok = run(args.only, args.reps, args.batch, lambda s: print(s, flush=True))
    sys.exit(0 if ok else GATE_FAILED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_timing.txt"))
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
            sys.exit(f"rows_timing: workload {name} ended with status {res.returncode}")
        ok = ok and res.returncode == 0
        out = res.stdout.splitlines()
        lines += out if not lines else out[1:]                    # the header once
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
