#!/usr/bin/env python3
"""N3Tree.subdivide / N3Tree.unshare (csrc/svoxt_subdivide.hip + the row gather) against the same steps written with
torch ops on the same GPU -- what a user did by hand before: refine(sel=...) with its host-side selection, then index
arithmetic for the new rows and features[row_map] -- on

    D8: the headline tree (synth depth 8, SH9 K = 28)
    C4: the config-4 tree (synth depth 9, K = 32)

    subdivide   subdivide(weights=, threshold=) with the threshold at the 90 % quantile of the non-empty leaves' weights:
                about 10 % of them split, each into N^3 leaves with rows of their own
    unshare     unshare() after a full refine(): every row named by N^3 leaves

Medians of event timings; every repetition works on a fresh copy of the tree, made outside the timed region.  Each
(tree, step) pair runs in a child process of its own under `timeout`; the first one that fails ends the run.

    python scripts/subdivide_timing.py [--reps 7] [--only D8] [--out profiles/subdivide_timing.txt]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TREES = {"D8": (8, 28, "SH9"), "C4": (9, 32, "RGBA")}
STEPS = ("subdivide", "unshare")
STEP_TIMEOUT = 420                                               # seconds per child


def torch_subdivide(tree, weights, threshold):
    """The baseline: select on the device, bring the list to the host as refine() does, refine, number the new rows."""
    import torch
    n, M, N = tree.n_internal, tree.features.shape[0], tree.N
    n3 = N ** 3
    pick = (tree.child[:n] == 0) & (tree.data[:n, ..., 0] >= 0) & (tree.data[:n, ..., 0] < M) & (weights[:n] >= threshold)
    leaves = pick.nonzero(as_tuple=False).cpu()                  # refine()'s selection lives on the host (_all_leaves)
    keep = tree.parent_depth[leaves[:, 0].to(tree.parent_depth.device), 1].cpu() < tree.depth_limit
    leaves = leaves[keep].to(tree.data.device)
    rows = tree.data[tuple(leaves.T)][:, 0].long()
    tree.refine(sel=tuple(leaves.T))
    added = leaves.shape[0]
    fresh = M + torch.arange(added * (n3 - 1), device=rows.device).reshape(added, n3 - 1)
    tree.data[n:n + added].reshape(added, n3)[:, 1:] = fresh.int()
    row_map = torch.cat((torch.arange(M, device=rows.device), rows.repeat_interleave(n3 - 1)))
    tree.features = torch.nn.Parameter(tree.features.detach()[row_map])
    return row_map


def torch_unshare(tree):
    """The baseline: a stable sort of the leaves' rows finds the first slot of every row."""
    import torch
    n, M = tree.n_internal, tree.features.shape[0]
    flat = tree.data[:n].reshape(-1)
    names = ((tree.child[:n].reshape(-1) == 0) & (flat >= 0) & (flat < M)).nonzero().squeeze(1)
    rows = flat[names].long()
    order = torch.argsort(rows, stable=True)
    srt = rows[order]
    later = torch.ones_like(srt, dtype=torch.bool)
    later[0] = False
    later[1:] = srt[1:] == srt[:-1]
    move = names[order[later]].sort().values
    row_map = torch.cat((torch.arange(M, device=rows.device), flat[move].long()))
    flat[move] = (M + torch.arange(move.shape[0], device=rows.device)).int()
    tree.features = torch.nn.Parameter(tree.features.detach()[row_map])
    return row_map


def timed(prep, fn, reps):
    import torch
    ts = []
    for i in range(reps + 1):                                    # the first repetition warms up
        x = prep()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(x)
        b.record()
        torch.cuda.synchronize()
        if i:
            ts.append(a.elapsed_time(b))
        del x
    ts.sort()
    return ts[len(ts) // 2]


def child_main(name, step, reps):
    import torch
    import svox_t_amd as svox
    from svox_t_amd import synth
    depth, K, fmt = TREES[name]
    dev = torch.device("cuda:0")
    st = synth.shell_tree(depth)
    base = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, synth.shell_features(st.n_features, K), data_format=fmt, device=dev)
    base.features.requires_grad_(False)
    n, M = base.n_internal, base.features.shape[0]
    tables = lambda t: (t.child[:t.n_internal], t.data[:t.n_internal], t.parent_depth[:t.n_internal], t.features.detach())   # noqa: E731
    same = lambda x, y: all(torch.equal(u, v) for u, v in zip(tables(x), tables(y)))                                         # noqa: E731
    if step == "subdivide":
        w = torch.rand(base.child.shape, device=dev, generator=torch.Generator(dev).manual_seed(0))
        full = (base.child == 0) & (base.data[..., 0] != svox.svox.EMPTY_INDEX)
        thr = float(w[full][:4_000_000].quantile(0.9))
        a, b = base.clone(), base.clone()
        res = a.subdivide(weights=w, threshold=thr)
        ok = same(a, b) if torch.equal(res.row_map, torch_subdivide(b, w, thr)) else False
        c = base.clone()
        rerun = torch.equal(c.subdivide(weights=w, threshold=thr).row_map, res.row_map) and same(a, c)
        t_hip = timed(base.clone, lambda t: t.subdivide(weights=w, threshold=thr), reps)
        t_topo = timed(base.clone, lambda t: t.subdivide(weights=w, threshold=thr, own_rows=False), reps)
        t_torch = timed(base.clone, lambda t: torch_subdivide(t, w, thr), max(3, reps // 2))
        print(f"{name} subdivide: depth {depth} K={K}  nodes {n} -> {a.n_internal} (+{res.nodes_added})  rows {M} -> {M + res.rows_added}  "
              f"equals the torch-ops result {ok}  run-to-run equal {rerun}")
        print(f"  hip   {t_hip:.3f} ms (own_rows=False, topology only: {t_topo:.3f} ms)   torch ops {t_torch:.3f} ms   -> {t_torch / t_hip:.1f}x")
        new_bytes = res.nodes_added * (2 * 8 * 4 + 12) + res.rows_added * 8 + 2 * (M + res.rows_added) * K * 4
        print(f"  bytes: {n * 8 * 12 / 2**20:.1f} MiB of tables and weights read by the mark pass, {n * 8 * 40 / 2**20:.1f} MiB of flags and "
              f"ranks through the scans and the list, {new_bytes / 2**20:.1f} MiB of new tables, row_map and the feature table read and written")
    else:
        base.refine()
        a, b = base.clone(), base.clone()
        res = a.unshare()
        ok = same(a, b) if torch.equal(res.row_map, torch_unshare(b)) else False
        c = base.clone()
        rerun = torch.equal(c.unshare().row_map, res.row_map) and same(a, c)
        del b, c
        t_hip = timed(base.clone, lambda t: t.unshare(), reps)
        t_rows = timed(lambda: (base.child, base.data.clone()), lambda x: svox.csrc.unshare_rows(x[0], x[1], base.n_internal, M), reps)
        t_torch = timed(base.clone, torch_unshare, max(3, reps // 2))
        print(f"{name} unshare after refine(): depth {depth} K={K}  nodes {base.n_internal}  rows {M} -> {M + res.rows_added}  "
              f"equals the torch-ops result {ok}  run-to-run equal {rerun}")
        print(f"  hip   {t_hip:.3f} ms (data words and row_map alone: {t_rows:.3f} ms)   torch ops {t_torch:.3f} ms   -> {t_torch / t_hip:.1f}x")
        print(f"  bytes: {base.n_internal * 8 * 8 * 2 / 2**20:.1f} MiB of child and data read twice, {2 * (M + res.rows_added) * K * 4 / 2**20:.1f} MiB "
              f"of feature rows read and written by the gather")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subdivide_timing.txt"))
    ap.add_argument("--child", nargs=2, metavar=("TREE", "STEP"))
    a = ap.parse_args()
    if a.child:
        return child_main(a.child[0], a.child[1], a.reps)
    lines = []
    for name in TREES:
        if a.only and a.only != name:
            continue
        for step in STEPS:
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps),
                   "--child", name, step]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            print(res.stdout, end="", flush=True)
            lines.append(res.stdout)
            if res.returncode != 0:                              # a fault, an abort or the time limit: nothing more runs
                print(f"{name} {step}: exit status {res.returncode}; stopping", flush=True)
                return res.returncode
    with open(a.out, "w") as f:
        f.write("python scripts/subdivide_timing.py (MI355X; medians of event timings, ms)\n" + "".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
