#!/usr/bin/env python3
"""N3Tree.set ("last" and "mean") and N3Tree.leaf_boxes (csrc/svoxt_assign.hip) against the same steps written with torch
ops on the same GPU -- query_vertical's data_ids plus index_put_ / scatter_reduce_ for set, nonzero plus the torch walk
of the parent chain (N3Tree._calc_corners as it was before the kernel) plus the gathers for leaf_boxes -- on

    C4: the config-4 tree (synth depth 9, K = 32)
    D8: the headline tree (synth depth 8, SH9 K = 28)

Points: 8 samples inside every occupied leaf ("leaf8", shuffled), and 1 M uniform points in the cube ("rand1m": most
fall into empty leaves of these shell trees), and 1 M points inside ONE occupied leaf ("one1m": a single group, walked
in its fixed order by one set of lanes).  Medians of event timings; the table is rewritten by every call, the
inputs are not.  Every step runs in a child process of its own under a time limit; the first one that fails ends the run.

    python scripts/assign_timing.py [--reps 7] [--only D8] [--limit 300]
"""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import svox_t_amd as svox                      # noqa: E402
from svox_t_amd import synth                   # noqa: E402

TREES = {"C4": (9, 32, "RGBA"), "D8": (8, 28, "SH9")}
STEPS = ["leaf_boxes", "last:leaf8", "mean:leaf8", "last:rand1m", "mean:rand1m", "mean:one1m"]


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def torch_corners(tree, nodes):
    """N3Tree._calc_corners with torch ops (a host read per level)."""
    corner = torch.zeros(nodes.shape[0], 3, device=nodes.device)
    curr = nodes.clone()
    live = torch.ones(nodes.shape[0], dtype=torch.bool, device=nodes.device)
    while True:
        corner[live] = (corner[live] + curr[:, 1:].float()) / tree.N
        up = curr[:, 0] != 0
        if not up.any():
            break
        idx = live.nonzero(as_tuple=False).squeeze(1)[up]
        live = torch.zeros_like(live)
        live[idx] = True
        curr = tree._unpack_index(tree.parent_depth[curr[up, 0], 0].long())
    return corner


def torch_leaf_boxes(tree):
    n, M = tree.filled, tree.features.shape[0]
    leaf_node = (tree.child[:n] == 0).nonzero(as_tuple=False)
    corners = (torch_corners(tree, leaf_node) - tree.offset) / tree.invradius
    depths = tree.parent_depth[leaf_node[:, 0], 1]
    lengths = (float(tree.N) ** (-depths.float() - 1.0))[:, None] / tree.invradius
    words = tree.data[:n].reshape(n, tree.N, tree.N, tree.N)[tuple(leaf_node.T)].long()
    return leaf_node, corners, lengths, depths, torch.where((words >= 0) & (words < M), words, torch.full_like(words, -1))


def torch_set(tree, table, pts, vals, mode):
    ids = tree.forward(table, pts, want_data_ids=True)[1]
    ok = ids >= 0
    if mode == "last":                                   # (which of a row's points lands is undefined)
        table.index_put_((ids[ok],), vals[ok])
    else:                                                # (float atomics: the sum depends on the order of arrival)
        table.scatter_reduce_(0, ids[ok][:, None].expand(-1, table.shape[1]), vals[ok], "mean", include_self=False)


def run_step(name, step, reps):
    depth, K, fmt = TREES[name]
    dev = torch.device("cuda:0")
    st = synth.shell_tree(depth)
    M = st.n_features
    tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, synth.shell_features(M, K), data_format=fmt, device=dev)
    head = f"{name} depth {depth} K={K} nodes {st.n_internal} rows {M}: {step:12s}"
    if step == "leaf_boxes":
        got, want = tree.leaf_boxes(), torch_leaf_boxes(tree)
        same = all(torch.equal(a, b) for a, b in zip(got, want))
        t, b = timed(tree.leaf_boxes, reps), timed(lambda: torch_leaf_boxes(tree), max(3, reps // 2))
        t_c = timed(lambda: svox.csrc.leaf_corners(tree.child, tree.parent_depth, 2, got.leaf_node), reps)
        b_c = timed(lambda: torch_corners(tree, got.leaf_node), max(3, reps // 2))
        print(f"{head} hip {t:.3f} ms  torch {b:.3f} ms  -> {b / t:.1f}x   the corners alone: hip {t_c:.3f} ms  torch {b_c:.3f} ms  -> "
              f"{b_c / t_c:.1f}x   leaves {got.leaf_node.shape[0]}  equal the torch-ops result {same}", flush=True)
        return
    mode, pset = step.split(":")
    gen = torch.Generator().manual_seed(1)
    if pset == "leaf8":
        lb = tree.leaf_boxes()
        idx = (lb.rows >= 0).nonzero().squeeze(1).repeat(8)
        idx = idx[torch.randperm(idx.shape[0], device=dev)]
        pts = (lb.corners[idx] + torch.rand((idx.shape[0], 3), device=dev) * lb.lengths[idx]).contiguous()
        del lb, idx
    elif pset == "one1m":
        lb = tree.leaf_boxes()
        i = int((lb.rows >= 0).nonzero()[0])
        pts = (lb.corners[i] + torch.rand((1 << 20, 3), device=dev) * lb.lengths[i]).contiguous()
        del lb
    else:
        pts = torch.rand((1 << 20, 3), generator=gen).to(dev)
    Q = pts.shape[0]
    vals = torch.randn((Q, K), device=dev)
    table = synth.shell_features(M, K, seed=2).to(dev)
    ref = table.clone()
    hip = lambda: tree.set(pts, vals, reduce=mode, features=table)       # noqa: E731
    hip()
    first = table.clone()
    rows, counts = tree.set(pts, vals, reduce=mode, features=table, return_rows=True)
    rerun = torch.equal(first, table)
    torch_set(tree, ref, pts, vals, mode)
    if mode == "last":      # with duplicates index_put_ keeps any one of a row's points: compare the rows that got exactly one
        one = rows[counts == 1]
        err = float((table[one] - ref[one]).abs().max()) if one.numel() else 0.0
        note = f"rows with one point equal torch's {err == 0.0} ({one.numel()} of {rows.numel()})"
    else:
        note = f"max |difference| to torch's atomics {float((table - ref).abs().max()):.2e}"
    t, b = timed(hip, reps), timed(lambda: torch_set(tree, ref, pts, vals, mode), max(3, reps // 2))
    print(f"{head} hip {t:.3f} ms  torch {b:.3f} ms  -> {b / t:.1f}x   points {Q}  rows written {rows.numel()}  "
          f"largest group {int(counts.max()) if counts.numel() else 0}  {note}  run-to-run equal {rerun}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--limit", type=int, default=300, help="seconds a step's child process may take")
    ap.add_argument("--step", default="", help="(internal) run this one step in this process")
    a = ap.parse_args()
    if a.step:
        return run_step(a.only, a.step, a.reps)
    for name in TREES:
        if a.only and a.only != name:
            continue
        for step in STEPS:
            rc = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--only", name,
                                 "--step", step, "--reps", str(a.reps)]).returncode
            if rc != 0:
                print(f"{name} {step}: ended with status {rc}; nothing further is run", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
