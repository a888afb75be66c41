#!/usr/bin/env python3
"""quantize_median_cut (svoxt_quant.hip) and what a palette does to the headline render, measured.

(a) the HIP pipeline on the headline tree's feature table (synth depth 8, SH9: 668 912 rows x 28 floats), order = 16,
    unweighted and weighted, against the same level-by-level algorithm written with torch ops on the same GPU (two
    stable torch.sort calls per level = a sort on the composite key (segment, value, row); segment_reduce for the
    extremes, the cuts and the means; cumsum for the weight prefixes and the new segment table; one host read per level
    for the segment count).  The torch-ops version is the comparison and is checked to give the same result.
    Context, not measured by this script: the reference's single-threaded CPU recursion (quantizer.cpp) took 17.9 s
    unweighted and 30.0 s weighted on this table, one run each on a CPU.
(b) the headline workload (bench.py's d8_sh9_800: 800 x 800 rays, forward and forward + backward of a fixed upstream
    gradient, image_shape hint) rendered from the full table and from the order = 16 and order = 12 palettes: same
    tree, rays and gradient; at least 1.5 s of untimed steps, then medians of per-step event timings.

    python scripts/quantize_timing.py [--reps 10] [--steps 60] [--out profiles/quantize_timing.txt]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import svox_t_amd as svox                      # noqa: E402
from svox_t_amd import csrc as _C              # noqa: E402
from svox_t_amd import synth                   # noqa: E402


def torch_quantize(data, weights, order):
    """The level-by-level median cut with torch ops; returns (colors, color_id_map)."""
    M, K = data.shape
    dev = data.device
    rows_all = torch.arange(M, device=dev)
    perm, row_seg = rows_all, torch.zeros(M, dtype=torch.long, device=dev)
    starts = torch.tensor([0, M], device=dev)
    w64 = weights.double() if weights is not None else None
    for _ in range(order):
        lens = starts[1:] - starts[:-1]
        S = lens.shape[0]
        rows = data[perm]
        mn = torch.segment_reduce(rows, "min", lengths=lens, unsafe=True)
        mx = torch.segment_reduce(rows, "max", lengths=lens, unsafe=True)
        is_open = lens > 1
        rng = torch.where(is_open[:, None], mx - mn, torch.zeros_like(mx))
        col = torch.argmax(rng, dim=1)
        val = data[rows_all, col[row_seg]] + 0.0
        i1 = torch.sort(val, stable=True).indices                        # (value, row)
        perm = i1[torch.sort(row_seg[i1], stable=True).indices]          # (segment, value, row)
        l, r = starts[:-1], starts[1:]
        if w64 is None:
            m = l + (r - l) // 2
        else:
            seg = row_seg[perm]
            run = torch.cat((torch.zeros(1, dtype=torch.float64, device=dev), torch.cumsum(w64[perm], 0)))
            pre = run[1:] - run[l][seg]
            tot = run[r] - run[l]
            first = torch.where(pre > 0.5 * tot[seg], rows_all, r[seg]).double()
            m = torch.segment_reduce(first, "min", lengths=lens, unsafe=True)
            m = torch.where(lens > 0, m, r.double()).long()
        n_out = torch.where(is_open, 2, 1)
        slot = torch.cumsum(n_out, 0) - n_out
        total = int(n_out.sum())                                         # the one host read of a level
        new = torch.empty(total + 1, dtype=torch.long, device=dev)
        new[slot] = l
        new[slot[is_open] + 1] = m[is_open]
        new[total] = M
        seg = row_seg[perm]
        row_seg = torch.empty_like(row_seg)
        row_seg[perm] = slot[seg] + (is_open[seg] & (rows_all >= m[seg])).long()
        starts = new
    lens = starts[1:] - starts[:-1]
    S = lens.shape[0]
    rows = data[perm].double()
    plain = torch.segment_reduce(rows, "sum", lengths=lens, unsafe=True) / lens[:, None]
    if w64 is not None:
        ws = w64[perm]
        tw = torch.segment_reduce(ws, "sum", lengths=lens, unsafe=True)
        mean = torch.segment_reduce(rows * ws[:, None], "sum", lengths=lens, unsafe=True) / tw[:, None]
        mean = torch.where((tw == 0)[:, None], plain, mean)
    else:
        mean = plain
    colors = torch.zeros((1 << order, K), device=dev)
    colors[:S] = torch.where((lens > 0)[:, None], mean, torch.zeros_like(mean)).float()
    return colors, row_seg.int()


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
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantize_timing.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    depth, K, W, H = 8, 28, 800, 800
    st = synth.shell_tree(depth)
    M = st.n_features
    feats = synth.shell_features(M, K).to(dev)
    weights = (torch.randint(0, 4097, (M,), device=dev, generator=torch.Generator(dev).manual_seed(0)) / 1024.0).float()
    say(f"(a) quantize_median_cut, {M} rows x {K} float32 ({M * K * 4 / 2**20:.1f} MiB), order = 16; medians of {a.reps} event timings (min .. max)")
    for name, w in (("unweighted", None), ("weighted  ", weights)):
        got = _C.quantize_median_cut(feats, w, 16)
        again = _C.quantize_median_cut(feats, w, 16)
        ref = torch_quantize(feats, w, 16)
        same_ids = torch.equal(got[1], ref[1])
        ulp = float(((got[0] - ref[0]).abs() / torch.clamp(ref[0].abs(), min=1e-30)).max()) / 2.0 ** -23
        rerun = torch.equal(got[1], again[1]) and torch.equal(got[0].view(torch.int32), again[0].view(torch.int32))
        t_hip = timed(lambda: _C.quantize_median_cut(feats, w, 16), a.reps)
        t_torch = timed(lambda: torch_quantize(feats, w, 16), max(3, a.reps // 2))
        say(f"  {name}  hip {t_hip[0]:.2f} ms ({t_hip[1]:.2f} .. {t_hip[2]:.2f})   torch ops {t_torch[0]:.2f} ms ({t_torch[1]:.2f} .. {t_torch[2]:.2f})"
            f"   -> {t_torch[0] / t_hip[0]:.1f}x   ids equal the torch-ops result {same_ids}, colours within {ulp:.2f} relative 2^-23; run-to-run equal {rerun}")
    say("  context (not measured here): the reference's CPU recursion, one run each on a CPU: 17.9 s unweighted, 30.0 s weighted")

    Q = W * H
    o, d, v = synth.pinhole_rays(W, H, c2w=synth.camera_pose(azimuth_deg=30.0))
    rays = svox.Rays(o.to(dev), d.to(dev), v.to(dev))
    say(f"(b) headline workload: depth {depth} SH9, {W} x {H} rays, image_shape hint; medians of {a.steps} steps after >= 1.5 s of untimed steps")
    base = None
    for name, order in (("full table      ", None), ("order 16 palette", 16), ("order 12 palette", 12)):
        tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, synth.shell_features(M, K), data_format="SH9", device=dev)
        if order is not None:
            tree.quantize(order)
        renderer = svox.VolumeRenderer(tree)
        features = tree.features
        gout = synth.grad_output(Q, 4).to(dev)

        def step(backward, events=None):
            features.grad = None
            if events is not None:
                events[0].record()
            if backward:
                out = renderer(features, rays, image_shape=(H, W))
                if events is not None:
                    events[1].record()
                out.backward(gout)
            else:
                with torch.no_grad():
                    renderer(features, rays, image_shape=(H, W))
            if events is not None:
                events[2].record()

        res = {}
        for backward in (False, True):
            t0 = time.time()
            while time.time() - t0 < 1.5:
                for _ in range(10):
                    step(backward)
                torch.cuda.synchronize()
            evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.steps)]
            for e in evs:
                step(backward, e)
            torch.cuda.synchronize()
            ts = sorted(e[0].elapsed_time(e[2]) for e in evs)
            res[backward] = ts[len(ts) // 2]
            if backward:
                fs = sorted(e[0].elapsed_time(e[1]) for e in evs)
                res["fwd_of_step"] = fs[len(fs) // 2]
        if base is None:
            base = res
        say(f"  {name} ({features.shape[0]:>6} rows, {features.numel() * 4 / 2**20:5.1f} MiB)  forward only {res[False]:.3f} ms ({res[False] / base[False]:.3f} of full)"
            f"   forward + backward {res[True]:.3f} ms ({res[True] / base[True]:.3f} of full; its forward {res['fwd_of_step']:.3f} ms)"
            f"   {Q / res[True] / 1e3:.1f} Mrays/s")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
