#!/usr/bin/env python3
"""RaySamples.split and merge_samples (csrc/svoxt_cut.hip) beside the same computation in PyTorch ops, on the same GPU,
lists and tensors in one process per workload, on the two benchmark workloads

    D8: the headline workload (synth depth 8, SH9, K = 28, 800 x 800)
    C4: the config-4 tree (synth depth 9, K = 32, 1024 x 1024)

per workload, on the lists of ray_samples(min_sigma = 0):
 (a) split(max_length) at the max_length that doubles the sample count, beside the piece counts as element-wise ops,
     repeat_interleave, the arithmetic of the pieces, four index-selects and the new offsets (cumsum + gather).
                                                                                                    GATE: HIP <= PyTorch
 (b) merge_samples with the lists of the same rays through a second synth tree of the same depth with another centre,
     beside the same union in PyTorch ops: the breakpoints of both lists sorted by (ray, z), the coverage of every
     interval between two neighbours of a ray found by searchsorted in each list, the covered intervals filtered
     (nonzero + index-selects), the new offsets (index_add + cumsum).                               GATE: HIP <= PyTorch
 not gated: split beside ray_samples, merge_samples beside the two marches.
The script exits with status 1 if a gate fails.  Every figure is the median of `--reps` event timings of `--batch` steps
each, taken after warm-up rounds that go on until two consecutive rounds agree within 3 %.  Without --only every workload
runs in a process of its own, under its own time limit, and the lines are written to profiles/cut_timing.txt.

    python scripts/cut_timing.py [--reps 9] [--batch 10] [--only D8]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"D8": (8, 28, "SH9", 800), "C4": (9, 32, "RGBA", 1024)}
WARM_UP = (5, 28, "SH9", 64)
SECOND_CENTER = (0.56, 0.47, 0.52)              # the second tree: same depth and radius, moved
GATE_FAILED = 3
LIMIT_S = 400                                   # a workload's process
MAX_PIECES = 4096


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


def torch_split(s, max_length):
    import torch
    T = len(s)
    mf = torch.ceil(s.length / torch.tensor(max_length, device=s.length.device))    # (a tensor: by a Python number torch multiplies with the reciprocal)
    m = torch.where((s.length > 0) & (mf >= 1), mf.clamp(max=float(MAX_PIECES)), torch.ones_like(mf)).long()
    ends = torch.cumsum(m, 0)
    index = torch.repeat_interleave(torch.arange(T, device=m.device), m)
    p = torch.arange(index.shape[0], device=m.device) - (ends - m)[index]
    mi = m[index]
    step = s.length[index] / mi.float()
    depth = torch.where(mi == 1, s.depth[index], s.depth[index] + p.float() * step)
    pos = torch.cat([ends.new_zeros(1), ends])
    return pos[s.offsets.clamp(0, T)], s.ray[index], s.row[index], depth, step, index


def torch_merge(a, b):
    import torch
    Q, dev = a.Q, a.ray.device
    big = 64.0                                                   # ray * big + z in float64 (z < 64): monotone along a list
    lists = []
    for s in (a, b):
        ray = s.ray.long()
        lists.append((ray, s.depth, s.depth + s.length, ray.double() * big + s.depth.double()))
    z = torch.cat([x for (_, st, en, _) in lists for x in (st, en)])
    ray = torch.cat([x for (r, _, _, _) in lists for x in (r, r)])
    order = torch.argsort(ray.double() * big + z.double())        # by (ray, z)
    z, ray = z[order], ray[order]
    lo, hi = z[:-1], z[1:]
    mid = ray[:-1].double() * big + 0.5 * (lo.double() + hi.double())
    live = (ray[:-1] == ray[1:]) & (hi > lo)
    index = []
    for (r, st, en, key) in lists:
        if key.shape[0] == 0:
            index.append(torch.full_like(ray[:-1], -1))
            continue
        at = torch.searchsorted(key, mid, right=True) - 1
        k = at.clamp(min=0)
        inside = (at >= 0) & (r[k] == ray[:-1]) & (0.5 * (lo + hi) < en[k])
        index.append(torch.where(inside, k, torch.full_like(k, -1)))
    keep = torch.nonzero(live & ((index[0] >= 0) | (index[1] >= 0)))[:, 0]
    ray_o = ray[:-1].index_select(0, keep)
    depth, length = lo.index_select(0, keep), (hi - lo).index_select(0, keep)
    ia, ib = index[0].index_select(0, keep), index[1].index_select(0, keep)
    counts = torch.zeros(Q, dtype=torch.int64, device=dev).index_add_(0, ray_o, torch.ones_like(ray_o))
    offsets = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=offsets[1:])
    return offsets, ray_o.int(), torch.full_like(ray_o, -1, dtype=torch.int32), depth, length, ia, ib


def run(name, reps, batch, say):
    import torch
    import svox_t_amd as svox
    from svox_t_amd import synth
    depth, K, fmt, W = WORKLOADS.get(name, WARM_UP)
    st = synth.shell_tree(depth)
    feats = synth.shell_features(st.n_features, K, seed=0)
    tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, data_format=fmt, device="cuda")
    second = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, data_format=fmt, center=SECOND_CENTER, device="cuda")
    r, r2 = svox.VolumeRenderer(tree), svox.VolumeRenderer(second)
    o, d, v = synth.pinhole_rays(W, W, c2w=synth.camera_pose())
    rays = svox.Rays(o.cuda(), d.cuda(), v.cuda())
    Q, shape = W * W, (W, W)

    t_lists = timed(lambda: r.ray_samples(rays, min_sigma=0.0, image_shape=shape), reps, batch)
    t_lists2 = timed(lambda: r2.ray_samples(rays, min_sigma=0.0, image_shape=shape), reps, batch)
    s = r.ray_samples(rays, min_sigma=0.0, image_shape=shape)
    s2 = r2.ray_samples(rays, min_sigma=0.0, image_shape=shape)
    T = len(s)

    # the max_length that doubles the sample count: bisection on the piece count
    lo, hi = 0.0, float(s.length.max())
    for _ in range(40):
        ml = 0.5 * (lo + hi)
        n = int(torch.ceil(s.length / ml).clamp(1, MAX_PIECES).sum())
        lo, hi = (ml, hi) if n > 2 * T else (lo, ml)
    ml = hi
    fine, fine_index = s.split(ml)
    t_split, t_torch_split = timed(lambda: s.split(ml), reps, batch), timed(lambda: torch_split(s, ml), reps, batch)
    same = all(torch.equal(x, y) for x, y in zip(torch_split(s, ml), (fine.offsets, fine.ray, fine.row, fine.depth, fine.length, fine_index)))

    m, ia, ib = svox.merge_samples(s, s2)
    t_merge, t_torch_merge = timed(lambda: svox.merge_samples(s, s2), reps, batch), timed(lambda: torch_merge(s, s2), reps, batch)
    n_torch = int(torch_merge(s, s2)[0][-1])
    ok_a, ok_b = t_split <= t_torch_split, t_merge <= t_torch_merge
    say(f"{name}: depth {depth}, K = {K}, {W} x {W} rays; {T} samples with sigma > 0, {T / Q:.1f} a ray, the longest list {int(s.counts.max())}; "
        f"the second tree (centre {SECOND_CENTER}): {len(s2)} samples")
    say(f"  (a) split(max_length = {ml:.6g}): {len(fine)} pieces             {t_split:8.3f} ms")
    say(f"      counts + repeat_interleave + arithmetic + 4 index + offsets  {t_torch_split:8.3f} ms   HIP / PyTorch = {t_split / t_torch_split:.2f}   "
        f"gate (<= 1): {'holds' if ok_a else 'FAILS'}   (the same arrays: {same})")
    say(f"  (b) merge_samples: {len(m)} pieces, {int(((ia >= 0) & (ib >= 0)).sum())} under both trees, the longest list {int(m.counts.max())}"
        f"      {t_merge:8.3f} ms")
    say(f"      sort by (ray, z) + 2 searchsorted + filter + offsets ({n_torch} pieces) {t_torch_merge:8.3f} ms   HIP / PyTorch = {t_merge / t_torch_merge:.2f}   "
        f"gate (<= 1): {'holds' if ok_b else 'FAILS'}")
    say(f"  ray_samples(min_sigma = 0), the first tree / the second         {t_lists:8.3f} / {t_lists2:8.3f} ms   split / ray_samples = {t_split / t_lists:.2f}, "
        f"merge / both marches = {t_merge / (t_lists + t_lists2):.2f}   (not gated)")
    return ok_a and ok_b


def one_workload(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("cut_timing: needs a GPU (a timing taken anywhere else says nothing)")
    print(f"cut_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}", flush=True)
    run("warm-up", 1, 1, lambda s: None)
    ok = run(args.only, args.reps, args.batch, lambda s: print(s, flush=True))
    sys.exit(0 if ok else GATE_FAILED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cut_timing.txt"))
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
            sys.exit(f"cut_timing: workload {name} ran into its limit of {LIMIT_S} s; nothing more is started")
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode not in (0, GATE_FAILED):
            sys.exit(f"cut_timing: workload {name} ended with status {res.returncode}; nothing more is started")
        ok = ok and res.returncode == 0
        out = res.stdout.splitlines()
        lines += out if not lines else out[1:]                    # the header once
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
