#!/usr/bin/env python3
"""N3Tree.prune's pipeline (csrc.prune_tree + csrc.gather_rows: svoxt_prune.hip) against the same four steps written
with torch ops on the same GPU (a port of tests/prune_restate.py: the baseline, what a user did by hand before), on

    C4: the config-4 tree (synth depth 9, K = 32: 792 753 nodes, 4 738 568 rows = 578 MiB)
    D8: the headline tree (synth depth 8, SH9 K = 28: 123 841 nodes, 668 912 rows)

with a random 50 % of the leaves kept, nodes collapsed, with and without feature compaction.  Medians of event timings
over fresh calls (the inputs are not modified).  Also: the row gather alone three ways (own kernel,
svoxt_permute_rows, torch indexing), and the compulsory bytes -- tables read and written once, kept rows read and
written once -- as a fraction of 8 TB/s.

    python scripts/prune_timing.py [--reps 10] [--only D8]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svox_t_amd import csrc as _C              # noqa: E402
from svox_t_amd import synth                   # noqa: E402

EMPTY = 1410065408
HBM = 8e12


def torch_prune(child, data, pd, n, M, keep, features, compact):
    """drop / collapse level by level / cumsum renumbering / row compaction with torch ops (collapse=True)."""
    N = child.shape[1]
    n3 = N ** 3
    ch = child[:n].reshape(n, n3).long()
    da = data[:n].reshape(n, n3).long()
    p = pd[:n].long()
    leaf = ch == 0
    full = leaf & (da >= 0) & (da < M)
    da = torch.where(full & ~keep[:n].reshape(n, n3), torch.full_like(da, EMPTY), da)
    full = full & keep[:n].reshape(n, n3)
    below = full.any(1).int()
    depth = p[:, 1]
    for d in range(int(depth.max()), 0, -1):                     # a host read, then a pass per level
        at = (depth == d).nonzero().squeeze(1)
        below.index_add_(0, p[at, 0] // n3, below[at])
    stays = below > 0
    stays[0] = True
    ids = torch.arange(n, device=ch.device)[:, None]
    kid = torch.where(leaf, torch.zeros_like(ch), ids + ch)
    gone = ~leaf & ~stays[kid]
    ch = torch.where(gone, torch.zeros_like(ch), ch)
    new_id = torch.cumsum(stays, 0) - 1
    inner = ch != 0
    ch = torch.where(inner, new_id[kid] - new_id[:, None], ch)
    da = torch.where(inner | gone, torch.full_like(da, EMPTY), da)
    p0 = new_id[p[:, 0] // n3] * n3 + p[:, 0] % n3
    p0[0] = p[0, 0]
    ch, da = ch[stays], da[stays]
    pd_out = torch.stack((p0, p[:, 1]), 1)[stays].int()
    row_map = feats = None
    if compact:
        full = (ch == 0) & (da < M)
        used = torch.zeros(M, dtype=torch.bool, device=ch.device)
        used[da[full]] = True
        row_map = used.nonzero().squeeze(1)
        rank = torch.cumsum(used, 0) - 1
        da = torch.where(full, rank[da.clamp(0, M - 1)], da)
        feats = features[row_map]
    return ch.int().reshape(-1, N, N, N), da.int().reshape(-1, N, N, N, 1), pd_out, int(ch.shape[0]), row_map, feats


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, depth, K in (("C4", 9, 32), ("D8", 8, 28)):
        if a.only and a.only != name:
            continue
        st = synth.shell_tree(depth)
        n, M = st.n_internal, st.n_features
        child = torch.from_numpy(st.child).to(dev)
        data = torch.from_numpy(st.data).to(dev)
        pd = torch.from_numpy(st.parent_depth).to(dev)
        feats = synth.shell_features(M, K).to(dev)
        keep = torch.rand(child.shape, device=dev, generator=torch.Generator(dev).manual_seed(0)) < 0.5

        def hip(compact):
            c, d, p, n2, rm = _C.prune_tree(child, data, pd, n, M, keep=keep, compact_features=compact)
            return c, d, p, n2, rm, (_C.gather_rows(feats, rm) if compact else None)

        def same(x, y):
            return all(torch.equal(u, v) for u, v in zip(x[:3] + x[4:], y[:3] + y[4:])) and x[3] == y[3]

        got = hip(True)
        ok, rerun = same(got, torch_prune(child, data, pd, n, M, keep, feats, True)), same(got, hip(True))
        n2, rm = got[3], got[4]
        M2 = rm.shape[0]
        t_topo, t_full = timed(lambda: hip(False), a.reps), timed(lambda: hip(True), a.reps)
        b_topo = timed(lambda: torch_prune(child, data, pd, n, M, keep, feats, False), max(3, a.reps // 2))
        b_full = timed(lambda: torch_prune(child, data, pd, n, M, keep, feats, True), max(3, a.reps // 2))
        rm32, dst = rm.int(), torch.empty((M2, K), device=dev)
        g_own = timed(lambda: _C.gather_rows(feats, rm), a.reps)
        g_perm = timed(lambda: _C._call("svoxt_permute_rows", feats.data_ptr(), rm32.data_ptr(), dst.data_ptr(), M2, K, 0,
                                        _C._stream(dev)), a.reps)
        g_torch = timed(lambda: feats[rm], a.reps)
        n3 = child.shape[1] ** 3
        table_bytes = (n + n2) * (2 * n3 * 4 + 8) + n * n3 * keep.element_size()      # child, data, parent_depth in and out; the decision
        row_bytes = 2 * M2 * K * 4 + M2 * 8
        floor_topo, floor_full = table_bytes / HBM * 1e3, (table_bytes + row_bytes) / HBM * 1e3
        print(f"{name}: depth {depth} K={K}  nodes {n} -> {n2}  rows {M} -> {M2}  equals the torch-ops result {ok}  run-to-run equal {rerun}")
        print(f"  hip   topology only {t_topo:.3f} ms   with feature compaction {t_full:.3f} ms")
        print(f"  torch (the same steps as tensor ops, nodes collapsed too) topology only {b_topo:.3f} ms   with feature compaction {b_full:.3f} ms   -> {b_topo / t_topo:.1f}x / {b_full / t_full:.1f}x")
        print(f"  row gather alone ({M2} rows of {K * 4} B): own kernel {g_own:.3f} ms  svoxt_permute_rows {g_perm:.3f} ms  "
              f"torch indexing {g_torch:.3f} ms  (own kernel: {2 * M2 * K * 4 / g_own / 1e9:.2f} TB/s read + written)")
        print(f"  compulsory bytes: tables {table_bytes / 2**20:.1f} MiB = {floor_topo:.4f} ms at 8 TB/s ({floor_topo / t_topo:.3f} of the topology time); "
              f"with rows {(table_bytes + row_bytes) / 2**20:.1f} MiB = {floor_full:.4f} ms ({floor_full / t_full:.3f} of the whole)", flush=True)


if __name__ == "__main__":
    main()
