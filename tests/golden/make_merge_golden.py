"""Regenerate tests/golden/merge_*.npz: what the REFERENCE's own Python (svox_t/svox.py:352-483, 600-642, run on the
CPU) makes of the topology_* trees -- its _frontier, max_frontier(), diam_frontier(), and the tables after
merge(mask, op=torch.max) + shrink_to_fit().

    python tests/golden/make_merge_golden.py /path/to/the/reference/checkout

Nothing of the reference is kept here, only the arrays it returns.  Its frontier code reads the int32 `data` words as
VALUES (that is what is stale about it in this fork), so the trees are given data_dim = 1 and a distinct word per leaf:
the reference then reduces and merges those words, and the tests read the same numbers as a one-column feature table
(features[w] = w).  max and the diameter of integers below 2^24 are exact in float32, so the fixtures pin values, not
tolerances; the tables after the merge pin the topology half (which nodes go, the renumbering, child offsets, packed
parent slots) word for word.

The tree is shrunk to fit first: _frontier combines a mask over n_internal nodes with one over the capacity.  The
reference lists the root in _frontier when all the root's slots are leaves (and merge() then refuses it); none of
these trees has such a root, which the generator asserts."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TREES = ["shell_d3", "shell_d4", "points_a", "full_n2_l3", "full_n3_l2"]


def main(ref_root):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref_root)
    warnings.simplefilter("ignore")
    import svox_t                                     # the reference; its extension is absent: the tensor-op paths run

    for name in TREES:
        g = np.load(os.path.join(HERE, f"topology_{name}.npz"))
        n = int(g["n_internal"])
        child, pd = g["child"][:n], g["parent_depth"][:n]
        N = child.shape[1]
        rng = np.random.default_rng(n)
        leaf = np.nonzero(child.reshape(-1) == 0)[0]
        words = np.zeros(child.size, np.int32)
        words[leaf] = rng.permutation(leaf.size)       # a distinct word per leaf, in no order
        data = words.reshape(n, N, N, N, 1)

        t = svox_t.N3Tree(N=N, data_dim=1, init_reserve=n + 1000)
        t.child[:n] = torch.from_numpy(child)
        t.data.data[:n] = torch.from_numpy(data)
        t.parent_depth[:n] = torch.from_numpy(pd)
        t._n_internal.fill_(n)
        t._invalidate()
        assert t.shrink_to_fit() and t.capacity == n
        frontier = t._frontier.numpy().copy()
        assert frontier.size and frontier[0] != 0, name
        mask = rng.random(frontier.size) < 0.5
        fmax = t.max_frontier().numpy().copy()
        fdiam = t.diam_frontier().numpy().copy()
        assert t.merge(torch.from_numpy(mask), op=torch.max)
        assert t.shrink_to_fit()
        n2 = t.n_internal
        assert n2 == n - int(mask.sum()) == t.capacity
        print(f"{name}: N = {N}, n = {n}, leaves = {leaf.size}, frontier = {frontier.size}, merged = {int(mask.sum())}, n' = {n2}")
        np.savez_compressed(os.path.join(HERE, f"merge_{name}.npz"), child=child, data=data, parent_depth=pd,
                            frontier=frontier.astype(np.int64), mask=mask, max_frontier=fmax.astype(np.int32),
                            diam_frontier=fdiam.astype(np.float32), child_after=t.child.numpy(),
                            data_after=t.data.data.numpy(), parent_depth_after=t.parent_depth.numpy())


if __name__ == "__main__":
    main(sys.argv[1])
