"""The *_workspace_bytes queries of the tree operators, without a GPU: callers allocate by them and each unit documents
the layout behind its size, so the sizes are held to the values recorded in tests/golden/workspace_bytes.json
(tests/golden/make_workspace_golden.py: the smallest legal extents, small ones, and those of synth.shell_tree(8))."""
import json
import os

import pytest

import svox_t_amd.csrc as _C
from tests.golden.make_workspace_golden import ask, cases

with open(os.path.join(os.path.dirname(__file__), "golden", "workspace_bytes.json")) as f:
    GOLDEN = json.load(f)


def test_the_golden_file_covers_the_generators_cases():
    assert [(g["query"], g["args"]) for g in GOLDEN] == [(q, a) for q, a in cases()]
    assert {g["query"] for g in GOLDEN} == {
        "svoxt_prune_workspace_bytes", "svoxt_merge_workspace_bytes", "svoxt_subdivide_workspace_bytes",
        "svoxt_frontier_workspace_bytes", "svoxt_neighbors_workspace_bytes", "svoxt_tv_plan_workspace_bytes",
        "svoxt_tv_workspace_bytes", "svoxt_assign_workspace_bytes", "svoxt_quantize_workspace_bytes",
        "svoxt_p2v_workspace_bytes", "svoxt_build_workspace_bytes",
        "svoxt_ray_samples_workspace_bytes", "svoxt_samples_select_workspace_bytes", "svoxt_samples_split_workspace_bytes",
        "svoxt_samples_merge_workspace_bytes", "svoxt_row_plan_workspace_bytes", "svoxt_reduce_rows_workspace_bytes",
        "svoxt_shade_samples_bwd_workspace_bytes", "svoxt_interp_rows_bwd_workspace_bytes",
        "svoxt_render_grad_rows_workspace_bytes"}


@pytest.mark.parametrize("g", GOLDEN, ids=lambda g: g["query"][6:-16] + "-" + "-".join(str(a) for a in g["args"] if not isinstance(a, list)))
def test_workspace_bytes_are_the_recorded_ones(g):
    got = ask(_C._lib, g["query"], g["args"])
    assert got == g["bytes"]


def test_four_queries_written_out():
    """Prune / merge (n, M), subdivide (n, 2, M) and frontier (n) at the three extents, in the test itself: the file and the
    generator cannot drift together unnoticed."""
    want = {"svoxt_prune_workspace_bytes": (9472, 13568, 6351616), "svoxt_merge_workspace_bytes": (2048, 6912, 7830272),
            "svoxt_subdivide_workspace_bytes": (1536, 16896, 19816704), "svoxt_frontier_workspace_bytes": (768, 1280, 991488)}
    for i, (n, M) in enumerate([(1, 0), (100, 500), (123841, 668912)]):
        assert _C._lib.svoxt_prune_workspace_bytes(n, M) == want["svoxt_prune_workspace_bytes"][i]
        assert _C._lib.svoxt_merge_workspace_bytes(n, M) == want["svoxt_merge_workspace_bytes"][i]
        assert _C._lib.svoxt_subdivide_workspace_bytes(n, 2, M) == want["svoxt_subdivide_workspace_bytes"][i]
        assert _C._lib.svoxt_frontier_workspace_bytes(n) == want["svoxt_frontier_workspace_bytes"][i]


def test_list_producer_queries_written_out():
    """The four list producers (svoxt_listemit.h: one carve for all of them) at the headline workload's 640 000 rays and
    5.9 M samples, in the test itself.  Per ray: a 64-bit total, Q counts, Q starts, the scan's chunk sums; per sample:
    T + 1 of each, select without the total (256 bytes less than split)."""
    Q, T = 640000, 5900000
    assert _C._lib.svoxt_ray_samples_workspace_bytes(Q) == 5121024
    assert _C._lib.svoxt_samples_merge_workspace_bytes(Q) == 5121024
    assert _C._lib.svoxt_samples_select_workspace_bytes(T) == 47206144
    assert _C._lib.svoxt_samples_split_workspace_bytes(T) == 47206400
    for query in ("svoxt_ray_samples_workspace_bytes", "svoxt_samples_merge_workspace_bytes", "svoxt_samples_select_workspace_bytes",
                  "svoxt_samples_split_workspace_bytes"):
        assert getattr(_C._lib, query)(0) == 0 and getattr(_C._lib, query)(-1) == -1 and getattr(_C._lib, query)(1 << 31) == -1
