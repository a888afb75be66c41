"""Regenerate tests/golden/workspace_bytes.json: what the *_workspace_bytes queries of the tree operators and of the
per-sample family answer, recorded from the library that is loaded (SVOXT_LIB names another build than the in-tree one):

    SVOXT_LIB=/path/to/libsvoxt_hip.so python tests/golden/make_workspace_golden.py

The sizes are part of what callers rely on (they allocate by them, and the layouts behind them are documented per unit),
so a change of the carving code must leave them as they are: tests/test_workspace_host.py holds the in-tree library to
this file.  Three argument sets per query: the smallest legal one, a small one, and the extents of synth.shell_tree(8)
(123 841 nodes, 990 728 slots, 866 888 leaves, 668 912 feature rows)."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "workspace_bytes.json")
NM = [(1, 0), (100, 500), (123841, 668912)]            # (n_internal, M)
LEAVES = [0, 500, 866888]
POINTS = [0, 100, 200000]
# (rays, samples, feature rows, K, colour channels, basis values a ray); the last is the headline workload (640 000 rays,
# 5.9 M samples, synth.shell_tree(8)'s rows of 28 floats: SH, 3 channels of 9).  CHUNKS: chunks of long rows, at most
# T / 256 + T / 257 of them.
SAMPLES = [(1, 1, 1, 1, 0, 0), (100, 500, 100, 4, 3, 0), (640000, 5900000, 668912, 28, 3, 9)]
CHUNKS = [1, 2, 5900000 // 256 + 5900000 // 257]


def cases():
    """(query, args): a list argument stands for a float32 array passed by pointer."""
    out = []
    for n, M in NM:
        out += [("svoxt_prune_workspace_bytes", [n, M]), ("svoxt_merge_workspace_bytes", [n, M]),
                ("svoxt_subdivide_workspace_bytes", [n, 2, M]), ("svoxt_frontier_workspace_bytes", [n]),
                ("svoxt_neighbors_workspace_bytes", [n, 2])]
    out += [("svoxt_subdivide_workspace_bytes", [100, 3, 500]), ("svoxt_neighbors_workspace_bytes", [100, 3])]
    for L, E in zip(LEAVES, [0, 700, 2000000]):
        out += [("svoxt_tv_plan_workspace_bytes", [L, -1]), ("svoxt_tv_plan_workspace_bytes", [L, E])]
    for M, cols in [(0, 1), (500, 4), (668912, 28)]:
        out.append(("svoxt_tv_workspace_bytes", [M, cols]))
    for Q, (_, M) in zip(POINTS, NM):
        out += [("svoxt_assign_workspace_bytes", [Q, M, reduce]) for reduce in range(5)]
    for M, K, order in [(1, 1, 0), (500, 4, 3), (668912, 28, 16)]:
        out += [("svoxt_quantize_workspace_bytes", [M, K, order, weighted]) for weighted in (0, 1)]
    for P, n_voxels, radius in [(0, 2, 0.0), (100, 16, 0.25), (200000, 128, 0.05)]:
        out.append(("svoxt_p2v_workspace_bytes", [P, n_voxels, [-1.0, -1.0, -1.0], [2.0, 2.0, 2.0], radius]))
    out += [("svoxt_build_workspace_bytes", [depth]) for depth in (1, 4, 8)]
    # the per-sample family: the smallest legal extents, small ones, the headline workload's
    for (Q, T, M, K, C, bd), chunks in zip(SAMPLES, CHUNKS):
        out += [("svoxt_ray_samples_workspace_bytes", [Q]), ("svoxt_samples_select_workspace_bytes", [T]),
                ("svoxt_samples_split_workspace_bytes", [T]), ("svoxt_samples_merge_workspace_bytes", [Q]),
                ("svoxt_row_plan_workspace_bytes", [T, M]), ("svoxt_reduce_rows_workspace_bytes", [chunks, K]),
                ("svoxt_shade_samples_bwd_workspace_bytes", [chunks, K]), ("svoxt_interp_rows_bwd_workspace_bytes", [chunks, K]),
                ("svoxt_render_grad_rows_workspace_bytes", [Q, T, M, K, C, bd])]
    return out


def ask(lib, query, args):
    keep = [(ctypes.c_float * len(a))(*a) if isinstance(a, list) else a for a in args]
    return int(getattr(lib, query)(*keep))


def main():
    import svox_t_amd.csrc as _C
    rows = [{"query": q, "args": a, "bytes": ask(_C._lib, q, a)} for q, a in cases()]
    assert all(r["bytes"] > 0 for r in rows), [r for r in rows if r["bytes"] <= 0]
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} sizes from {_C.LIB_PATH} -> {OUT}")


if __name__ == "__main__":
    main()
