#!/usr/bin/env python3
"""N3Tree.leaf_neighbors / the edge plan / tv / tv_add_grad (csrc/svoxt_neighbors.hip) against the same quantities written
with PyTorch ops, on the same GPU in one process, on the two benchmark trees

    D8: the headline tree (synth depth 8, SH9, K = 28)
    C4: the config-4 tree (synth depth 9, K = 32)

with weight="uniform", p = 2, dim=None and dim=-1:
    (a) leaf_neighbors            torch: a float probe point per face through forward(want_node_ids=True), searchsorted
    (b) the plan build            torch: the edge list (row_i, row_j) from that table with masks and index arithmetic
    (c) tv forward + backward per step, warm plan      torch: index_select differences, autograd
    (d) tv_add_grad               torch: (c) and grad.add_(g, alpha=scale)
(a), (b): one call each on a fresh tree (they are cached per topology), host clock around a synchronise, after a small
tree has been through every call once (code objects, allocator).  (c), (d): the median of
`--reps` event timings of `--batch` calls each, after a warm-up.  Beside (c): the bytes it has to move -- 2E K' 4 gathered
+ M K' 4 read + M K 4 written -- over its time, against the 8 TB/s HBM roof.  Writes profiles/tv_timing.txt.

    python scripts/tv_timing.py [--reps 9] [--batch 10] [--only D8]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import svox_t_amd as svox                      # noqa: E402
from svox_t_amd import synth                   # noqa: E402

TREES = {"D8": (8, 28, "SH9"), "C4": (9, 32, "RGBA")}
WARM_UP = (5, 28, "SH9")        # a small tree through every call first: code objects loaded, allocator and libraries warm
HBM = 8e12


def timed(fn, reps, batch):
    for _ in range(batch):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / batch)
    return sorted(ts)[len(ts) // 2]


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def torch_neighbors(tree):
    """The neighbour table by float probes: the centre of the cell across each face through the point query."""
    boxes = tree.leaf_boxes(world=False)
    L, N = boxes.depths.shape[0], tree.N
    step = torch.zeros(6, 3, device=boxes.corners.device)
    for k in range(6):
        step[k, k // 2] = 1.0 if k % 2 else -1.0
    probes = (boxes.corners[:, None, :] + boxes.lengths[:, None, :] * (0.5 + step[None])).reshape(-1, 3)
    inside = ((probes >= 0) & (probes < 1)).all(1)
    _, ids = tree(tree.features.detach(), probes.clamp(0, 1 - 1e-7).contiguous(), want_node_ids=True, world=False)
    slots = boxes.leaf_node[:, 0] * N ** 3 + (boxes.leaf_node[:, 1] * N + boxes.leaf_node[:, 2]) * N + boxes.leaf_node[:, 3]
    j = torch.searchsorted(slots, ids).reshape(L, 6)
    finer = boxes.depths[j.clamp(max=L - 1)] > boxes.depths[:, None]
    nb = torch.where(finer, torch.full_like(j, -2), j)
    return torch.where(inside.reshape(L, 6), nb, torch.full_like(j, -1)), boxes


def torch_edges(nb, boxes):
    i, k = (nb >= 0).nonzero(as_tuple=True)
    j = nb[i, k]
    di, dj, ri, rj = boxes.depths[i], boxes.depths[j], boxes.rows[i], boxes.rows[j]
    edge = ((dj < di) | ((dj == di) & (k % 2 == 1))) & (ri >= 0) & (rj >= 0) & (ri != rj)
    return ri[edge].contiguous(), rj[edge].contiguous()


def run(name, reps, batch, say):
    depth, K, fmt = TREES.get(name, WARM_UP)
    st = synth.shell_tree(depth)
    feats = synth.shell_features(st.n_features, K, seed=0)
    tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, data_format=fmt, device="cuda")
    M = tree.features.shape[0]
    nb, t_a = once(tree.leaf_neighbors)
    plan, t_b = once(lambda: tree._tv_plan(M))
    (tnb, boxes), t_ta = once(lambda: torch_neighbors(tree))
    (ri, rj), t_tb = once(lambda: torch_edges(tnb, boxes))
    L, E = nb.neighbors.shape[0], plan.E
    same = bool(torch.equal(tnb.int(), nb.neighbors)) and int(ri.shape[0]) == E
    say(f"{name}: depth {depth}, K = {K}, M = {M} rows, L = {L} leaves, E = {E} edges, plan {plan.nbytes / 1e6:.1f} MB; "
        f"torch's table and edge count equal the kernel's: {same}")
    say(f"  (a) leaf_neighbors   {t_a:9.2f} ms   torch probes {t_ta:9.2f} ms   x{t_ta / t_a:.1f}")
    say(f"  (b) plan build       {t_b:9.2f} ms   torch edges  {t_tb:9.2f} ms   x{t_tb / t_b:.1f}")
    for dim in (None, -1):
        Kc = K if dim is None else 1
        cols = slice(None) if dim is None else slice(K - 1, K)
        f = tree.features

        def ours():
            f.grad = None
            tree.tv(dim=dim).backward()

        def theirs():
            f.grad = None
            d = f.index_select(0, ri)[:, cols] - f.index_select(0, rj)[:, cols]
            (d * d).sum().backward()

        acc = torch.zeros_like(f)

        def ours_add():
            tree.tv_add_grad(acc, 1e-3, dim=dim)

        def theirs_add():
            theirs()
            acc.add_(f.grad, alpha=1e-3)

        ours()
        g1 = f.grad.clone()
        theirs()
        err = float((g1 - f.grad).abs().max() / f.grad.abs().max())
        t_c, t_tc, t_d, t_td = (timed(fn, reps, batch) for fn in (ours, theirs, ours_add, theirs_add))
        moved = 4.0 * (2 * E * Kc + M * Kc + M * K)
        say(f"  dim={dim}: gradient against torch's: max |difference| / max |g| = {err:.2e}")
        say(f"  (c) tv fwd + bwd     {t_c:9.3f} ms   torch        {t_tc:9.3f} ms   x{t_tc / t_c:.2f}   "
            f"{moved / 1e6:.1f} MB -> {moved / t_c / 1e9:.3f} TB/s, {100 * moved / (t_c * 1e-3) / HBM:.1f} % of the 8 TB/s roof")
        say(f"  (d) tv_add_grad      {t_d:9.3f} ms   torch        {t_td:9.3f} ms   x{t_td / t_d:.2f}")
    del tree


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=sorted(TREES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tv_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tv_timing: needs a GPU (a timing taken anywhere else says nothing)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tv_timing: {torch.cuda.get_device_name(0)}, reps {args.reps}, batch {args.batch}; p = 2, weight = uniform")
    run("warm-up", 1, 1, lambda s: None)
    for name in ([args.only] if args.only else sorted(TREES, reverse=True)):
        run(name, args.reps, args.batch, say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
