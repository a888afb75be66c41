#!/usr/bin/env python3
"""The frontier reductions and N3Tree.merge (csrc/svoxt_merge.hip) against the same steps written with torch ops on the
same GPU -- nonzero for the frontier, an index gather to [F, 8, K], mean / pairwise norms, a table rewrite with
cumulative sums -- on

    C4: the config-4 tree (synth depth 9, K = 32)
    D8: the headline tree (synth depth 8, SH9 K = 28)

Steps: diam_frontier, reduce_frontier("mean"), merge of every frontier node, merge of the half of the frontier with the
smaller diameter.  Medians of event timings over fresh calls (the inputs are not modified).  Every step runs in a child
process of its own under a time limit; the first one that fails ends the run.

    python scripts/merge_timing.py [--reps 10] [--only D8] [--limit 240]
"""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svox_t_amd import csrc as _C              # noqa: E402
from svox_t_amd import synth                   # noqa: E402

EMPTY = 1410065408
TREES = {"C4": (9, 32), "D8": (8, 28)}
STEPS = ["diam", "mean", "merge_all", "merge_half"]


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


def torch_frontier(child, n):
    sel = (child[:n].reshape(n, -1) == 0).all(1)
    sel[0] = False
    return sel.nonzero().squeeze(1)


def torch_gather(feats, data, n, fr):
    words = data[:n].reshape(n, -1)[fr].long()
    has = (words >= 0) & (words < feats.shape[0])
    return feats[words.clamp(0, feats.shape[0] - 1)] * has[..., None], has, words


def torch_diam(feats, data, n, fr):
    rows, _, _ = torch_gather(feats, data, n, fr)
    return torch.cdist(rows, rows, compute_mode="donot_use_mm_for_euclid_dist").amax((1, 2))


def torch_merge(child, data, pd, n, feats, nodes):
    """merge of the frontier nodes `nodes` with mean / empty="zero" / compact_features as tensor ops."""
    M, n3 = feats.shape[0], child.shape[1] ** 3
    ch, da, p = child[:n].reshape(n, n3).long(), data[:n].reshape(n, n3).long(), pd[:n].long()
    rows, has, words = torch_gather(feats, data, n, nodes)
    takes = (words == words[:, :1]).all(1) | ~has.any(1)
    new_nodes = nodes[~takes]
    new_rows = rows[~takes].mean(1)
    stays = torch.ones(n, dtype=torch.bool, device=ch.device)
    stays[nodes] = False
    word_of = torch.zeros(n, dtype=torch.long, device=ch.device)
    word_of[nodes] = torch.where(takes, words[:, 0], torch.full_like(words[:, 0], -1))
    leaf = ch == 0
    used = torch.zeros(M + 1, dtype=torch.bool, device=ch.device)
    lw = da[stays][leaf[stays]]
    used[lw.clamp(0, M)] = True
    used[word_of[nodes][takes].clamp(0, M)] = True
    used = used[:M]
    row_map = used.nonzero().squeeze(1)
    rank = torch.cumsum(used, 0) - 1
    new_of = torch.zeros(n, dtype=torch.long, device=ch.device)
    new_of[new_nodes] = row_map.shape[0] + torch.arange(new_nodes.shape[0], device=ch.device)
    new_id = torch.cumsum(stays, 0) - 1
    ids = torch.arange(n, device=ch.device)[:, None]
    kid = torch.where(leaf, torch.zeros_like(ch), ids + ch)
    gone = ~leaf & ~stays[kid]
    w = torch.where(gone, word_of[kid], da)
    named = (leaf | gone) & (w >= 0) & (w < M)
    out_da = torch.where(named, rank[w.clamp(0, M - 1)], torch.where(leaf | (gone & (w != -1)), w, torch.full_like(w, EMPTY)))
    out_da = torch.where(gone & (w == -1), new_of[kid], out_da)
    out_ch = torch.where(leaf | gone, torch.zeros_like(ch), new_id[kid] - new_id[:, None])
    p0 = new_id[p[:, 0] // n3] * n3 + p[:, 0] % n3
    p0[0] = p[0, 0]
    N = child.shape[1]
    return (out_ch[stays].int().reshape(-1, N, N, N), out_da[stays].int().reshape(-1, N, N, N, 1),
            torch.stack((p0, p[:, 1]), 1)[stays].int(), int(stays.sum()), torch.cat((feats[row_map], new_rows)), row_map)


def run_step(name, step, reps):
    depth, K = TREES[name]
    dev = torch.device("cuda:0")
    st = synth.shell_tree(depth)
    n, M = st.n_internal, st.n_features
    child, data, pd = (torch.from_numpy(x).to(dev) for x in (st.child, st.data, st.parent_depth))
    feats = synth.shell_features(M, K).to(dev)
    fr = _C.frontier_nodes(child, n)
    F = fr.shape[0]
    head = f"{name} depth {depth} K={K} nodes {n} rows {M} frontier {F}: {step:10s}"
    if step in ("diam", "mean"):
        if step == "diam":
            hip, ref = (lambda: _C.frontier_diam(feats, data, n, 2, fr)), (lambda: torch_diam(feats, data, n, fr))
        else:
            hip, ref = (lambda: _C.frontier_reduce(feats, data, n, 2, fr, None, "mean")), (lambda: torch_gather(feats, data, n, fr)[0].mean(1))
        err = float((hip() - ref()).abs().max())
        t_f = timed(lambda: (_C.frontier_nodes(child, n), hip()), reps)
        b_f = timed(lambda: (torch_frontier(child, n), ref()), max(3, reps // 2))
        t, b = timed(hip, reps), timed(ref, max(3, reps // 2))
        read = F * 8 * 4 + M * K * 4
        print(f"{head} hip {t:.3f} ms  torch {b:.3f} ms  -> {b / t:.1f}x   with the frontier: hip {t_f:.3f} ms  torch {b_f:.3f} ms  -> {b_f / t_f:.1f}x   "
              f"max |difference| {err:.2e}   gathered tensor {F * 8 * K * 4 / 2**20:.0f} MiB; rows read once: {read / 2**20:.0f} MiB = {read / t / 1e9:.2f} TB/s",
              flush=True)
        return
    sel_idx = fr
    if step == "merge_half":
        d = _C.frontier_diam(feats, data, n, 2, fr)
        sel_idx = fr[d <= d.median()]
    selected = torch.zeros(n, dtype=torch.uint8, device=dev)
    selected[sel_idx] = 1
    hip = lambda: _C.merge_tree(child, data, pd, n, feats, selected, "mean", "zero", True, 0, EMPTY)      # noqa: E731
    ref = lambda: torch_merge(child, data, pd, n, feats, sel_idx)                                          # noqa: E731
    got, want = hip(), ref()
    same = all(torch.equal(got[i], want[i]) for i in (0, 1, 2, 5)) and got[3] == want[3]
    err = float((got[4] - want[4]).abs().max())
    again = hip()
    rerun = all(torch.equal(got[i], again[i]) for i in (0, 1, 2, 4, 5))
    t, b = timed(hip, reps), timed(ref, max(3, reps // 2))
    print(f"{head} hip {t:.3f} ms  torch {b:.3f} ms  -> {b / t:.1f}x   nodes -> {got[3]}  rows -> {got[4].shape[0]} ({got[6]} new)  "
          f"tables equal the torch-ops result {same}  max |row difference| {err:.2e}  run-to-run equal {rerun}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--limit", type=int, default=240, help="seconds a step's child process may take")
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
