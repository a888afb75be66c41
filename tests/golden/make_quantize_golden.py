"""Regenerate tests/golden/quantize_*.npz: inputs of quantize_median_cut and the outputs of the REFERENCE's own
quantize_median_cut (svox_t/csrc/quantizer.cpp, plain CPU code) on them.

    python tests/golden/make_quantize_golden.py /path/to/module.so

The argument is a Python extension module, built outside this repository, that binds the reference's function under
its own name -- quantize_median_cut(data, weights, order) -> (colors, color_id_map); nothing of it is kept here, only
the arrays it returns.

Every case is checked with the numpy restatement (tests/quantize_restate.py) before it is written: at every split
the winning column's range is a strict maximum and the values either side of the cut differ, so no tie-break -- the
one thing nth_element / sort leave open -- decides anything and the reference's color_id_map is the only correct one;
and the weights are small integers, so the reference's float32 running sums are exact.

weighted_dominant has one row that outweighs all others: where it sorts first its segment's left child is empty,
where it sorts second the left child has one row and closes levels early -- the case that pins the numbering of the
colours.  The reference's row for an empty segment is 0 / 0 = NaN (this project writes zeros there); the generator
checks that those are its only NaN rows."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import quantize_restate as R  # noqa: E402


def cases():
    rng = np.random.default_rng(20240607)
    yield "unweighted_k28", rng.standard_normal((1000, 28)).astype(np.float32), None, 6
    yield "unweighted_full", rng.standard_normal((256, 4)).astype(np.float32), None, 8
    yield "weighted_int", rng.standard_normal((900, 28)).astype(np.float32), rng.integers(1, 9, 900).astype(np.float32), 5
    w = np.ones(300, np.float32)
    w[137] = 4096.0                      # more than everything else together: every cut of its segment falls at its row
    for seed in range(1000):             # the first seed at which the heavy row sorts first somewhere: an empty child
        data = np.random.default_rng(seed).standard_normal((300, 7)).astype(np.float32)
        report = {}
        starts = R.quantize(data, w, 6, report)[3]
        if report["unique"] and (np.diff(starts) == 0).any():
            break
    yield "weighted_dominant", data, w, 6


def main(path):
    spec = importlib.util.spec_from_file_location(os.path.splitext(os.path.basename(path))[0], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name, data, weights, order in cases():
        report = {}
        _, ids, _, starts, _ = R.quantize(data, weights, order, report)
        assert report["unique"], f"{name}: a tie decides a split; pick another seed"
        wt = torch.from_numpy(weights) if weights is not None else torch.empty(0)
        colors, color_id_map = mod.quantize_median_cut(torch.from_numpy(data), wt, order)
        colors, color_id_map = colors.numpy(), color_id_map.numpy()
        lens = np.diff(starts)
        print(f"{name}: M = {data.shape[0]}, K = {data.shape[1]}, order = {order}, segments = {len(lens)}, "
              f"empty = {(lens == 0).sum()}, NaN rows = {np.isnan(colors).any(axis=1).sum()}, "
              f"ids equal the restatement's: {np.array_equal(ids, color_id_map)}")
        empty = np.zeros(1 << order, bool)
        empty[:len(lens)] = lens == 0
        assert np.array_equal(np.isnan(colors).any(axis=1), empty), f"{name}: a NaN colour that is not an empty segment's"
        assert np.array_equal(ids, color_id_map), name
        if name == "weighted_dominant":
            assert empty.any() and len(lens) < 1 << order and (colors[len(lens):] == 0).all()
        np.savez_compressed(os.path.join(HERE, f"quantize_{name}.npz"), data=data,
                            weights=weights if weights is not None else np.zeros(0, np.float32),
                            order=np.int32(order), colors=colors, color_id_map=color_id_map)


if __name__ == "__main__":
    main(sys.argv[1])
