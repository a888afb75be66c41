"""Regenerate tests/golden/subdivide_*.npz: what the REFERENCE's own Python (svox_t/svox.py:488-560, run on the CPU)
makes of the topology_* trees when half of their leaves are refined -- N3Tree.refine(sel=<the masked leaves in
lexicographic order>).

    python tests/golden/make_subdivide_golden.py /path/to/the/reference/checkout

Nothing of the reference is kept here, only the arrays it returns.  Every leaf gets a distinct data word (in no order),
so the tables after the refine pin which word every new slot inherits, next to the topology half: which slots split,
the new nodes in selector order, child offsets, packed parent slots, depths.  The mask is over the slots of `child`
(entries at inner slots are ignored); N3Tree.subdivide(mask, own_rows=False, split_empty=True) has to write the same
tables word for word.  The trees are shallower than the reference's depth_limit (10), so no selected leaf is held back,
which the generator asserts."""
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
        rng = np.random.default_rng(n + 1)
        leaf = np.nonzero(child.reshape(-1) == 0)[0]
        words = np.zeros(child.size, np.int32)
        words[leaf] = rng.permutation(leaf.size)       # a distinct word per leaf, in no order
        data = words.reshape(n, N, N, N, 1)
        mask = rng.random(child.shape) < 0.5           # over every slot: inner slots are ignored

        chosen = torch.from_numpy(mask & (child == 0)).nonzero(as_tuple=False)      # the masked leaves, lexicographic
        # room for the new nodes up front: the reference's regrowth synchronises a GPU (svox.py:855)
        t = svox_t.N3Tree(N=N, data_dim=1, init_reserve=n + chosen.shape[0] + 3)
        t.child[:n] = torch.from_numpy(child)
        t.data.data[:n] = torch.from_numpy(data)
        t.parent_depth[:n] = torch.from_numpy(pd)
        t._n_internal.fill_(n)
        t.filled = n
        t._invalidate()
        assert int(pd[:, 1].max()) < t.depth_limit
        t.refine(sel=tuple(chosen.T))
        n2 = t.n_internal
        assert n2 == n + chosen.shape[0] == t.filled
        print(f"{name}: N = {N}, n = {n}, leaves = {leaf.size}, split = {chosen.shape[0]}, n' = {n2}")
        np.savez_compressed(os.path.join(HERE, f"subdivide_{name}.npz"), child=child, data=data, parent_depth=pd, mask=mask,
                            child_after=t.child[:n2].numpy(), data_after=t.data.data[:n2].numpy(),
                            parent_depth_after=t.parent_depth[:n2].numpy())


if __name__ == "__main__":
    main(sys.argv[1])
