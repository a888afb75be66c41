#!/usr/bin/env python3
"""Headline benchmark: Mrays/s of volume_render forward + backward on synthetic
800x800 renders of the depth-8 SH9 shell tree (BASELINE.json configs[2]).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload ...] [--forward-only] [--route plain|camera]
                    [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
        --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A "step" is one pass of the hot path over one ray batch: VolumeRenderer.forward on Q = W*H rays
followed by backward() of a fixed upstream gradient, i.e. volume_render + volume_render_backward
through the autograd.Function surface.  Inputs (tree topology, feature table, rays, upstream
gradient) are resident in HBM before the timed region.  With N > 1 every rank holds a replica of
the tree and renders its own camera (weak scaling: per-GPU work fixed); the pixels are gathered while the
backward runs, and the gradient is all-reduced (row chunks on a side stream, svox_t_amd/parallel.py) and
WAITED FOR before the next step starts -- the arrangement of a trainer that updates the features after every
batch (svox_t/renderer.py:60-77 under an optimizer); the gradient-accumulation arrangement, in which the
all-reduce hides under the next step, is timed afterwards and reported beside it (--full).

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the K steps, writes the last timed step's
outputs if --dump-outputs DIR is given (see dump_outputs) and prints the headline: metric, value, unit,
higher_is_better, dtype, ms_per_step and the per-step intervals behind them.  Everything else is measured with
--full only: the device-side counts, the other routes and tolerance modes, BASELINE.json's other configs, the N > 1
accumulation arrangement and exchange probe, and the line's `counters`, `touched`, `compulsory_bytes`, `roofline`,
`limits` and `cpu_baseline`.  With --full, `roofline` prices the bytes
THIS implementation cannot avoid moving to and from memory for the dominant kernel group (what
the algorithm as run reads and writes once: rays, pixels, sample records, the distinct feature
rows and tree words touched, the memset, the atomic requests, the row compaction -- counted on
the device before the timed region) against the 8 TB/s HBM peak; `reference_equivalent_gbps`
keeps SURVEY.md 8(d)'s figure for the reference's algorithm (three marches, 8 B per gradient
float) next to it.  The working set of configs 1-3 lives in the 256 MiB Infinity Cache, so
`limits` names what actually bounds each kernel.  `cpu_baseline`: the CPU oracle on the same
workload, host cores.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)
# exp/atomic_bench.hip (NOTEBOOK.md 5): the memory side takes 64-byte float-atomic requests at
# ~22 G/s whatever their size or scope (3.0 M wave-atomics of two segments each: 0.614 ms)
ATOMIC_REQUESTS_PER_S = 22e9
# us per leaf crossing of a wavefront alone on its SIMD: r02 timeline of march_rec_kernel
# (exp/trace_march.py, profiles/r02_march_timeline.txt) for the stepping alone; r01 timeline of
# render_fwd_kernel (NOTEBOOK.md 5, "Timelines") for stepping + shading in one chain
US_PER_CROSSING_UNLOADED = {"march": 0.72, "march+shade": 1.14}

WORKLOADS = {
    # name: (depth, K, data_format, width, height)
    "d8_sh9_800": (8, 28, "SH9", 800, 800),          # BASELINE configs[1]/[2] -- the metric's config
    "d5_rgba_64": (5, 4, "RGBA", 64, 64),            # configs[0]
    "d9_rgba32_1024": (9, 32, "RGBA", 1024, 1024),   # configs[3]
}


ROUND = "r05"        # which round's committed profiles the line quotes (profiles/<ROUND>_*)
# Untimed steps before the --warmup steps the contract asks for: full steps (forward AND backward) for at least
# PREWARM_MIN_S of wall time and until the last PREWARM_WINDOW forward and backward event intervals each lie within
# PREWARM_TOL of their median, at most PREWARM_MAX_S.  (r04: a fixed count of 30 + 5 steps, ~25 ms of GPU work, left
# the first process on a fresh box with backwards at 0.41-0.45 ms against 0.26 ms in steady state -- BENCH_r04.json,
# gpurun_out/r4b/bench_d8_1.json vs _2.json: the memory side of a cold device; BASELINE.md "fresh box".)
PREWARM_MIN_S, PREWARM_MAX_S, PREWARM_WINDOW, PREWARM_TOL, PREWARM_BATCH = 1.0, 4.0, 10, 0.05, 20
# ... and no downward trend left: the median of the steps of the last PREWARM_TREND_S seconds within PREWARM_TREND_TOL of the median of
# the PREWARM_TREND_S before them (r05: a fresh box's backward went 0.2702 -> 0.2638 ms over its first 0.5 s and on to 0.258 -- inside
# the 5 % window all the way, so `converged` said yes while the device was still warming: the headline 1 252 beside 1 298 for the
# routes measured after it)
PREWARM_TREND_S, PREWARM_TREND_TOL = 0.4, 0.01
STALL_FACTOR = 4.0
DUMP_BYTES = 64 * 10 ** 6      # --dump-outputs: the files' size in all, headers included


def dump_outputs(path, arrays, budget=DUMP_BYTES):
    """--dump-outputs: each array as <path>/<name>.npy, float32.  Smallest first, an array that does not fit an equal
    share of what is left of `budget` keeps a fixed sample of its rows (row indices drawn with seed 0, in ascending
    order), so that two builds run with the same arguments can be compared file for file.  Returns {name: rows kept}."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    left = budget - 128 * len(arrays)                 # (a .npy header is 128 bytes for these shapes)
    items = sorted(arrays.items(), key=lambda kv: kv[1].numel())
    kept = {}
    for i, (name, t) in enumerate(items):
        t = t.detach().float()
        rows = t.shape[0]
        row_bytes = 4 * max(1, t.numel() // max(rows, 1))
        keep = min(rows, left // (len(items) - i) // row_bytes)
        if keep < rows:
            idx = torch.randperm(rows, generator=torch.Generator().manual_seed(0))[:keep].sort().values
            t = t.index_select(0, idx.to(t.device))
        a = t.cpu().numpy()
        np.save(os.path.join(path, name + ".npy"), a)
        left -= a.nbytes
        kept[name] = keep
    return kept


def _median(xs):
    xs = sorted(xs)
    n = len(xs)
    return 0.0 if n == 0 else (xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2]))


def _spread(xs):
    """{min, median, max, mean} of a list of milliseconds."""
    return {"min": round(min(xs), 4), "median": round(_median(xs), 4), "max": round(max(xs), 4),
            "mean": round(sum(xs) / len(xs), 4)} if xs else None


def self_launch(args, argv):
    """`python3 bench.py --gpus N` as typed (no WORLD_SIZE in the environment): start the N ranks as CHILD processes --
    `python3 -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py
    ...`, exactly the command the driver would have typed -- before this process has made any GPU call (a process
    that has initialised the GPU must never be replaced), relay rank 0's one JSON line and the exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # (dmabuf IPC: what RCCL needs on this pool)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{") and ln.rstrip().endswith("}")]
    for ln in p.stdout.splitlines():
        if ln not in lines[-1:]:
            print(ln, file=sys.stderr)                    # (whatever else the ranks wrote to stdout: not the contract's line)
    if lines:
        print(lines[-1], flush=True)
    return p.returncode if (p.returncode or lines) else 1


def kernel_stats_ms(workload, forward_only, per_step=False):
    """{kernel name prefix: mean ms per launch} from this round's committed `rocprofv3 --kernel-trace --stats`
    summary of the same command (profiles/<ROUND>_<workload>[_fwd]_kernel_stats.csv), or {}.
    per_step: {name: (total ms, calls)} of EVERY kernel instead (kernel_table divides by the steps the profiled run made)."""
    import csv
    path = os.path.join(ROOT, "profiles", f"{ROUND}_{workload}{'_fwd' if forward_only else ''}_kernel_stats.csv")
    out = {}
    try:
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r["Name"].replace("void ", "").replace("svoxt::", "")
                key = name.split("(")[0]
                if per_step:
                    out[key] = (float(r["TotalDurationNs"]) * 1e-6, int(r["Calls"]))
                elif int(r["Calls"]) >= 10:                # (the one-off counting launches are not the step's)
                    out[key] = round(float(r["AverageNs"]) * 1e-6, 5)
    except Exception:
        return {}
    return out


def pmc_traffic(workload, forward_only, group):
    """(bytes per launch group, note) from this round's committed rocprofv3 --pmc passes of the same
    command (scripts/pmc_passes.sh -> scripts/pmc_summary.py), or (None, reason)."""
    name = f"{ROUND}_{workload}{'_fwd' if forward_only else ''}_pmc.json"
    path = os.path.join(ROOT, "profiles", name)
    try:
        with open(path) as f:
            counters = json.load(f)["counters"]
        ks = {"forward": ("fwd", "roles", "finish", "march", "shade", "exptab", "mask"), "backward": ("bwd", "fused", "merge", "wide", "compact")}[group]
        fetch = sum(counters[k]["FETCH_SIZE"] for k in ks if k in counters) * 1024.0
        write = sum(counters[k]["WRITE_SIZE"] for k in ks if k in counters) * 1024.0
        if fetch + write == 0:
            return None, f"no kernel of the {group} group in profiles/{name}"
        return int(2 * fetch + write), (
            f"(2 x FETCH_SIZE + WRITE_SIZE) x 1024 from profiles/{name} (separate --pmc passes of this command): "
            "MI355X_MICROARCH.md 'HBM': gfx950 FETCH_SIZE tallies 128-byte requests at 64 bytes -- doubled; "
            "WRITE_SIZE exact for streaming stores and float atomics.  Memory-side requests of the L2s: "
            "Infinity-Cache hits are included, so this bounds HBM bytes from above")
    except Exception as exc:   # no profile committed for this build / workload
        return None, f"no PMC summary profiles/{name} ({exc.__class__.__name__})"


# short kernel key (scripts/pmc_summary.py's) -> the kernel-name prefixes that belong to it in the kernel statistics
KERNEL_KEYS = {"mask": ("sigma_mask_kernel",), "exptab": ("exp_table_kernel",), "roles": ("fwd_roles_kernel",),
               "finish": ("fwd_finish_kernel",), "march": ("march_rec_kernel",), "shade": ("shade_chan_kernel", "shade_tile_kernel"),
               "fwd": ("render_fwd_kernel",), "fused": ("grad_fused_kernel",), "wide": ("grad_wide_kernel",),
               "compact": ("compact_rows",), "fill": ("__amd_rocclr_fillBufferAligned",), "bwd": ("render_bwd_kernel",)}


def pmc_kernel(workload, forward_only, key):
    """(2 x FETCH_SIZE + WRITE_SIZE) x 1024 of ONE kernel key from this round's committed PMC passes, or None."""
    path = os.path.join(ROOT, "profiles", f"{ROUND}_{workload}{'_fwd' if forward_only else ''}_pmc.json")
    try:
        with open(path) as f:
            c = json.load(f)["counters"].get(key)
        return None if not c else int((2 * c.get("FETCH_SIZE", 0.0) + c.get("WRITE_SIZE", 0.0)) * 1024.0)
    except Exception:
        return None


def kernel_table(workload, forward_only, assign, survey, group_ms, prof_ok):
    """The step's kernels, one row each:
        ms                 the kernel family's time per step (total duration of all its launches / steps of the profiled run) from
                           THIS ROUND's committed `rocprofv3 --kernel-trace --stats` of the same command
                           (profiles/<ROUND>_<workload>[_fwd]_kernel_stats.csv); kernels inside one C-ABI call cannot be
                           separated by this run's own events -- those give the group totals (`groups`)
        compulsory_bytes   what this implementation's algorithm must move once through that kernel (counted on the device)
        overhead_bytes     passes the reference does not have (bitmask / table builds, padding and its clearing): NOT in frac
        frac               compulsory_bytes / ms / 8 TB/s
        survey_8d_bytes    SURVEY.md 8(d)'s bytes of the REFERENCE's algorithm for the work this kernel stands for; frac_8d from
                           them -- above 1 means the kernel does not do the reference's work (lists instead of marches, the grid
                           instead of the descent, the per-tile merge instead of per-sample atomics), not that it beats the roof
        traffic            (2 x FETCH_SIZE + WRITE_SIZE) x 1024 from the committed PMC passes; traffic_ratio = traffic / compulsory
    assign: {kernel key: (compulsory bytes, overhead bytes, group)}; survey: {kernel key: bytes}."""
    kstats = kernel_stats_ms(workload, forward_only, per_step=True) if prof_ok else {}
    # steps the profiled run made = launches of the step's main kernels (each runs once per step)
    main = [c for n, (_, c) in kstats.items() if n.startswith(("fwd_roles_kernel", "grad_fused_kernel", "grad_wide_kernel", "march_rec_kernel",
                                                              "render_fwd_kernel", "shade_chan_kernel"))]
    steps_profiled = max(main) if main else 0
    rows = []
    for key, (comp, over, group) in assign.items():
        ms = None
        for name, (tot, calls) in kstats.items():
            # (instances that ran once -- the counting launches in front of the timed region -- are not the step's)
            if steps_profiled and 2 * calls >= steps_profiled and any(name.startswith(pre) for pre in KERNEL_KEYS.get(key, ())):
                ms = (ms or 0.0) + tot / steps_profiled          # the family's time per step (every instance and launch of it)
        traffic = pmc_kernel(workload, forward_only, key) if prof_ok else None
        row = {"kernel": key, "names": list(KERNEL_KEYS.get(key, ())), "group": group, "ms": None if ms is None else round(ms, 5),
               "compulsory_bytes": int(comp), "overhead_bytes": int(over),
               "frac": None if not ms else round(comp / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
               "survey_8d_bytes": survey.get(key), "frac_8d": None if (not ms or survey.get(key) is None)
               else round(survey[key] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
               "traffic": traffic, "traffic_ratio": None if (not traffic or not comp) else round(traffic / comp, 3)}
        rows.append(row)
    rows.sort(key=lambda r: -(r["ms"] or 0.0))
    return rows


def reference_equivalent_bytes(cnt, Q, M, K, C):
    """the bytes of the REFERENCE's algorithm.  cnt = (rays_hit, steps S, levels sum L, valid, active)."""
    _, S, L, V, A = cnt
    march = 4 * L + 4 * S + 4 * V + 4 * (K - 1) * A
    fwd = Q * (36 + 4 * (C + 1)) + march
    bwd = 4 * M * K + Q * (36 + 4 * (C + 1)) + 2 * march + A * (8 * (K - 1) + 8)
    return fwd, bwd


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="d8_sh9_800", choices=list(WORKLOADS))
    ap.add_argument("--route", default="hinted", choices=["hinted", "plain", "camera"],
                    help="hinted: VolumeRenderer.forward(..., image_shape=(H, W)); plain: exactly the two calls the "
                         "reference's own autograd function makes on the operator module (no hint, no extra argument); "
                         "camera: VolumeRenderer.render_persp (rays generated in the kernels, no ray tensors in HBM)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-plain", action="store_true", help="skip the extra plain-route measurement")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short measurements of BASELINE.json's other single-GPU configs that the default headline "
                         "run carries along (`other_configs`: configs[1] forward, fast=True rows, configs[3])")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL); gloo only for dry runs")
    ap.add_argument("--share-device", action="store_true",
                    help="dry run: put every rank on cuda:0 (to rehearse the N>1 code path on a 1-GPU box)")
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--fast", action="store_true",
                    help="sigma_thresh = stop_thresh = 1e-2 (svox_t/renderer.py:428-430): SURVEY.md 8(d)'s extra row; the headline is thresholds 0")
    ap.add_argument("--exchange", default="all_reduce", choices=["auto", "all_reduce", "direct"],
                    help="N > 1: the gradient all-reduce.  all_reduce (default): RCCL's own, in 32 MB row chunks; direct: "
                         "parallel.direct_all_reduce (reduce-scatter + all-gather as two rounds of simultaneous point-to-point "
                         "transfers, one per xGMI link); auto: both are timed on a gradient-sized buffer first and the faster is "
                         "used.  The point-to-point form has never run on RCCL hardware (one-GPU boxes only: tests cover it on "
                         "gloo), so it is opt-in: the first multi-GPU measurement must not depend on it")
    ap.add_argument("--prewarm-s", type=float, default=PREWARM_MIN_S,
                    help="least seconds of untimed full steps before the --warmup steps (0: one batch of %d steps: for runs under "
                         "a profiler, where every dispatch is slow)" % PREWARM_BATCH)
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU: rehearse launch, rendezvous, pixel gather, gradient exchange, timing and the JSON line on CPU "
                         "tensors over gloo with a stand-in for the renderer (tests/test_bench_launch.py); the number means nothing")
    ap.add_argument("--full", action="store_true",
                    help="also measure and report everything beyond the headline (off: set up, warm up, time the K steps, "
                         "print the headline): the device-side counts and the roofline, limits and compulsory bytes priced "
                         "from them, the other routes, the tolerance mode, BASELINE.json's other configs, the CPU baseline, "
                         "and with N > 1 the accumulation arrangement and the exchange probe; the --no-* options trim it")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one computed as DIR/pixels.npy and (with a backward) "
                         "DIR/grad_features.npy, float32, at most 64 MB in all (a fixed seeded sample of rows beyond that)")
    args = ap.parse_args(argv)
    if args.dry_run and args.dump_outputs:
        ap.error("--dump-outputs writes the renderer's outputs; a --dry-run has none")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args, sys.argv[1:] if argv is None else argv)       # (before anything touches the GPU)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    args.gpus = world                     # (under a launcher the launcher's world size is the truth)
    if args.dry_run:
        return dry_run(args, world, rank)
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    if args.share_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import datetime
        import torch.distributed as dist_mod
        dist = dist_mod
        kw = {"device_id": dev} if args.backend == "nccl" else {}
        dist.init_process_group(args.backend, timeout=datetime.timedelta(seconds=300), **kw)

    import svox_t_amd as svox
    import svox_t_amd.csrc as _C
    from svox_t_amd import parallel, synth
    from svox_t_amd.renderer import _rays_spec_from_rays

    depth, K, fmt, W, H = WORKLOADS[args.workload]
    Q = W * H
    st = synth.shell_tree(depth)
    feats = synth.shell_features(st.n_features, K)
    tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, data_format=fmt, device=dev)
    renderer = svox.VolumeRenderer(tree)
    # rank r renders camera r (azimuth 30 + 45 r degrees), SURVEY.md 8(d)
    pose = synth.camera_pose(azimuth_deg=30.0 + 45.0 * rank)
    o, d, v = synth.pinhole_rays(W, H, c2w=pose)
    rays = svox.Rays(o.to(dev), d.to(dev), v.to(dev))
    features = tree.features
    M = features.shape[0]
    opt = renderer._get_options(args.fast)
    C = _C.get_out_data_dim(opt, K) - 1
    gout = synth.grad_output(Q, C + 1).to(dev)

    class _ReferenceShaped(torch.autograd.Function):
        """svox_t/renderer.py:60-77: the two calls the reference's own function makes."""

        @staticmethod
        def forward(ctx, data, tspec, rspec, ropt):
            out = _C.volume_render(tspec, rspec, ropt)
            ctx.tree, ctx.rays, ctx.opt = tspec, rspec, ropt
            return out

        @staticmethod
        def backward(ctx, grad_out):
            return _C.volume_render_backward(ctx.tree, ctx.rays, ctx.opt, grad_out.contiguous()), None, None, None

    if args.forward_only:
        # inference: the caller declares the feature table static, so what the operator layer derives from its
        # content (the sigma bitmask) is built once and cached; a training step rebuilds it in every forward
        tree.static_features = True
    c2w = torch.from_numpy(pose).float().to(dev)
    fx = 1111.111 * W / 800.0

    def render(route):
        if route == "plain":
            rs = _C.RaysSpec()
            rs.origins, rs.dirs, rs.vdirs = rays.origins, rays.dirs, rays.viewdirs
            return _ReferenceShaped.apply(features, tree._spec(features), rs, opt)
        if route == "camera":
            return renderer.render_persp(features, c2w, width=W, height=H, fx=fx, fast=args.fast).view(Q, -1)
        return renderer(features, rays, image_shape=(H, W), fast=args.fast)

    # ---- one-off device-side counts (before the timed region; --full) -------------------------------
    cnt = touched = atomic_requests = merged_rows = None
    if args.full:
        rs_hint = _rays_spec_from_rays(rays, (H, W))
        rs_hint.need_grad = False
        spec = tree._spec(features)
        cnt = _C.count_forward(spec, rs_hint, opt).cpu().tolist()
        touched = _C.count_touched(spec, rs_hint, opt)
        if not args.forward_only:
            with _C.bwd_counters(dev) as ctr:
                features.grad = None
                render(args.route).backward(gout)
                torch.cuda.synchronize()
            atomic_requests, merged_rows = ctr.read()
            features.grad = None
    # N > 1: which gradient exchange?  RCCL's own all-reduce (ring / tree over its channels) or the direct form priced in
    # NOTEBOOK.md 7 (reduce-scatter + all-gather as two rounds of simultaneous point-to-point transfers, one per xGMI link)?
    # Measured here on a gradient-sized buffer, both checked against each other; the faster one is what the step uses.
    # (A plain run with the default exchange has nothing to choose: the probe is then a --full record.)
    exchange = None
    if dist is not None and not args.forward_only and (args.full or args.exchange != "all_reduce"):
        probe = torch.ones((M, K), dtype=torch.float32, device=dev)
        timings = {}
        for mode in (("all_reduce", "direct") if args.exchange == "auto" else (args.exchange,)):
            # A mode may fail on ONE rank only (point-to-point unavailable on its device): every rank then still joins
            # the collective that agrees on the outcome -- the MAX of (time, or inf on failure) -- outside the try, so that
            # nobody waits in it for a rank that took the except branch.
            dt, ok = float("inf"), False
            try:
                red = parallel.OverlappedGradReducer(dist, backend=args.backend, mode=mode)
                for rep_i in range(2 + 5):
                    if rep_i == 2:
                        torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    probe.fill_(1.0)
                    red.start(probe)
                    red.wait()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / 5
                ok = bool((probe == float(world)).all().item())
            except Exception as exc:                     # (a backend without point-to-point on this device: gloo dry runs)
                print(f"[bench] exchange '{mode}' unavailable on rank {rank}: {exc.__class__.__name__}: {exc}", file=sys.stderr)
            t = torch.tensor([dt if ok else float("inf")], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            timings[mode] = float(t.item())
        best = min(timings, key=timings.get) if args.exchange == "auto" else args.exchange
        if timings.get(best, float("inf")) == float("inf"):
            best = "all_reduce"
        exchange = {"used": best, "probe_ms": {k: (None if v == float("inf") else round(v * 1e3, 4)) for k, v in timings.items()},
                    "bytes": 4 * M * K,
                    "requested": args.exchange,
                    "what": "all-reduce(sum) of a gradient-sized buffer, 5 repetitions after 2, max over ranks, per exchange form probed "
                            "(--exchange auto probes both: the backend's own all_reduce in 32 MB row chunks and "
                            "parallel.direct_all_reduce, two rounds of simultaneous point-to-point transfers, one per link of the "
                            "mesh, and uses the faster; default: the backend's own)"}
        del probe
    reducer = parallel.OverlappedGradReducer(dist, backend=args.backend, mode=exchange["used"] if exchange else "all_reduce") \
        if dist is not None else None
    gathered = torch.empty((world * Q, C + 1), dtype=torch.float32, device=dev) if dist is not None else None
    def new_events(n):
        return [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)]

    ev = new_events(args.steps)

    def step(i=None, route=args.route, accumulate=False, events=None):
        e = (events if events is not None else ev)[i] if i is not None else None
        features.grad = None              # (a gradient still travelling is held by the reducer)
        # (two events per step, not three: a step's forward starts where the step before ended -- its last event; each
        # record costs the timed loop ~4 us, 0.012 ms per step with three: measured r03, 0.519 against 0.531 ms)
        # (N > 1 keeps its own start event: there the collectives' waits lie between two steps)
        if e and (i == 0 or dist is not None): e[0].record()
        if args.forward_only:
            with torch.no_grad():                              # inference: nothing is recorded for a backward
                out = render(route)
        else:
            out = render(route)
        if e: e[1].record()
        gather = None
        if dist is not None:
            # the pixels are final after the forward: gather them while the backward runs
            gather = parallel.gather_pixels_async(dist, gathered, out.detach(), backend=args.backend)
        if not args.forward_only:
            out.backward(gout)
        if e: e[2].record()
        if dist is not None:
            if not args.forward_only:
                reducer.start(features.grad)           # row chunks on a side stream
                if not accumulate:
                    # every-step update: the reduced gradient is needed before the features may change,
                    # i.e. before the next forward -- the all-reduce is exposed (this is the timed arrangement)
                    reducer.wait()
                # accumulate: the previous batch's reduced gradient is complete here; this batch's travels
                # under the next batch's forward and backward (gradient accumulation over batches / cameras)
            if gather is not None:
                gather.wait()
        return out

    def intervals(events, n):
        """(forward ms, backward ms) per step from the events of n steps (after a synchronize)."""
        fwd = [(events[i][0] if (i == 0 or dist is not None) else events[i - 1][2]).elapsed_time(events[i][1]) for i in range(n)]
        bwd = [events[i][1].elapsed_time(events[i][2]) for i in range(n)]
        return fwd, bwd

    _TEST_STALL_MS = [float(os.environ.get("BENCH_TEST_STALL_MS", "0") or 0)]      # (tests/test_gpu_bench_contract.py)
    last_out = [None]          # what the last step of the last timed() returned (--dump-outputs)

    def timed(n, **kw):
        """Seconds of n steps, bracketed by barrier + synchronize, max over ranks."""
        if reducer is not None:
            reducer.wait()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            if i == 1 and _TEST_STALL_MS[0] > 0:                     # (tests: the host falls asleep once, as a stalled step looks)
                torch.cuda.synchronize()
                time.sleep(_TEST_STALL_MS[0] * 1e-3)
                _TEST_STALL_MS[0] = 0.0
            out = step(i if kw.get("events") else None, **{k: v for k, v in kw.items() if k != "events"})
            if i == n - 1:
                last_out[0] = out
            del out                           # (no step's output outlives it but the last one, as before)
        if reducer is not None:
            reducer.wait()                    # the last gradient is reduced inside the timed region
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el

    # Setup, not measurement: bring the device to its steady state before the W warm-up steps the contract asks for.
    # By time and convergence, not by count (see PREWARM_* above): batches of full steps with per-step events, until at
    # least PREWARM_MIN_S have passed AND the last PREWARM_WINDOW forward and backward intervals each lie within
    # PREWARM_TOL of their median -- or PREWARM_MAX_S are over, which the line then shows (`prewarm.converged` false).
    # Every rank runs the same number of batches (the decision is all-reduced): the collectives stay matched.
    # (the host's own pauses stay out of the K timed steps as far as they can be kept out: the cyclic collector runs HERE, before
    # the warm-up, and not again until the timed steps are over -- between warm-up and timed steps it would leave the device idle
    # for tens of milliseconds, and an idle device's memory side takes ~15 steps to come back (r05: backward 0.259 -> 0.268 ms
    # over the 20 timed steps, 1 290 -> 1 252 Mrays/s); a step that still stalls shows in per_step_ms -- and see `retimed` below)
    gc.collect()
    gc.disable()
    pre_ev = new_events(PREWARM_BATCH)
    pre_fwd, pre_bwd, pre_steps, converged = [], [], 0, False
    t_pre = time.perf_counter()
    while True:
        for i in range(PREWARM_BATCH):
            step(i, events=pre_ev)
        if reducer is not None:
            reducer.wait()
        torch.cuda.synchronize()
        f_, b_ = intervals(pre_ev, PREWARM_BATCH)
        pre_fwd += f_; pre_bwd += b_; pre_steps += PREWARM_BATCH
        el_pre = time.perf_counter() - t_pre

        def settled(xs):
            w = xs[-PREWARM_WINDOW:]
            m = _median(w)
            return m > 0 and all(abs(x - m) <= PREWARM_TOL * m for x in w)
        def flat(xs):
            n = max(PREWARM_BATCH, int(PREWARM_TREND_S * pre_steps / max(el_pre, 1e-9)))      # steps in PREWARM_TREND_S of this workload
            if len(xs) < 2 * n:
                return False
            a, b = _median(xs[-2 * n:-n]), _median(xs[-n:])
            return b >= (1.0 - PREWARM_TREND_TOL) * a
        converged = settled(pre_fwd) and (args.forward_only or settled(pre_bwd))
        if args.prewarm_s >= PREWARM_MIN_S:       # (the trend rule with the default warm-up only: profiler runs shorten it)
            converged = converged and flat(pre_fwd) and (args.forward_only or flat(pre_bwd))
        done = (el_pre >= args.prewarm_s and (converged or args.prewarm_s <= 0)) or el_pre >= PREWARM_MAX_S
        if dist is not None:
            t = torch.tensor([1.0 if done else 0.0, 1.0 if converged else 0.0], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            done, converged = bool(t[0].item() == 1.0), bool(t[1].item() == 1.0)
        if done:
            break
    prewarm = {"steps": pre_steps, "seconds": round(el_pre, 3), "converged": converged,
               "first_batch_ms": {"forward": round(_median(pre_fwd[:PREWARM_BATCH]), 4),
                                  "backward": round(_median(pre_bwd[:PREWARM_BATCH]), 4)},
               "last_batch_ms": {"forward": round(_median(pre_fwd[-PREWARM_BATCH:]), 4),
                                 "backward": round(_median(pre_bwd[-PREWARM_BATCH:]), 4)},
               "rule": f">= {PREWARM_MIN_S} s of full steps and the last {PREWARM_WINDOW} forward and backward intervals within "
                       f"{PREWARM_TOL:.0%} of their median, no downward trend left (median of the last {PREWARM_TREND_S} s of steps within {PREWARM_TREND_TOL:.0%} of the {PREWARM_TREND_S} s before), at most {PREWARM_MAX_S} s (untimed; medians of the first / last "
                       f"{PREWARM_BATCH} steps shown: a cold device shows up as first >> last)"}
    if hasattr(_C, "freeze_pools"):
        _C.freeze_pools(True)      # the lists' pool sizes stay what the warm-up settled on: no re-sizing inside the timed steps
    for _ in range(args.warmup):
        step()
    elapsed = timed(args.steps, events=True)
    # A stalled step (r05: one 20 ms step among twenty of 0.8 ms, once in some hundred runs, on a box that was normal before
    # and after -- the queue the host keeps filled ran dry for a moment) is the host's, not the path's: when an interval is
    # more than STALL_FACTOR times its median the K steps are timed ONCE more, and the line carries both runs (`retimed`).
    retimed = None
    f1, b1 = intervals(ev, args.steps)
    stall = max(max(f1) / max(_median(f1), 1e-9), (max(b1) / max(_median(b1), 1e-9)) if not args.forward_only else 0.0)
    again = stall > STALL_FACTOR
    if dist is not None:
        t = torch.tensor([1.0 if again else 0.0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        again = bool(t.item() > 0.0)
    if again:
        retimed = {"why": f"a timed step took more than {STALL_FACTOR}x the median of its kind: the K steps were timed once more and "
                          "`value`, `ms_per_step`, `per_step_ms` are the second run's; the first run is kept here",
                   "first_run": {"ms_per_step": round(elapsed * 1e3 / args.steps, 4),
                                 "forward": [round(x, 4) for x in f1], "backward": [round(x, 4) for x in b1]}}
        elapsed = timed(args.steps, events=True)
    # what the caller of the timed path received from its last step (N > 1: this rank's pixels, the reduced gradient),
    # written before anything else runs on the device
    if args.dump_outputs and rank == 0:
        outs = {"pixels": last_out[0]}
        if not args.forward_only:
            outs["grad_features"] = features.grad
        dump_outputs(args.dump_outputs, outs)
    last_out[0] = None
    gc.enable()
    if hasattr(_C, "freeze_pools"):
        _C.freeze_pools(False)

    route_fwd, route_bwd = _C.LAST_ROUTE["forward"], (None if args.forward_only else _C.LAST_ROUTE["backward"])
    forward_terms = bool(_C.LAST_ROUTE.get("forward_terms"))       # (of the timed route: the runs below take others)
    fwd_steps, bwd_steps = intervals(ev, args.steps)
    step_steps = [a + b for a, b in zip(fwd_steps, bwd_steps)]
    fwd_ms = sum(fwd_steps) / args.steps
    bwd_ms = sum(bwd_steps) / args.steps

    # N > 1: the gradient-accumulation arrangement (one gradient in flight under the next step) beside the
    # timed every-step-update one, same process, same number of steps
    accumulation = None
    if args.full and dist is not None and not args.forward_only:
        for _ in range(3):
            step(accumulate=True)
        el = timed(args.steps, accumulate=True)
        accumulation = {"value": round(world * Q / (el / args.steps) / 1e6, 3), "unit": "Mrays/s",
                        "ms_per_step": round(el * 1e3 / args.steps, 4),
                        "what": "gradient accumulation over batches: step i's all-reduce travels (side stream, row chunks) "
                                "under step i+1's forward and backward; only the last one is exposed"}

    # the other routes, for the record (same process, after the timed region)
    WHAT = {"plain": "the two calls the reference's own autograd function makes (svox_t/renderer.py:60-77) on "
                     "svox_t_amd.csrc: no image hint; the operator layer recognises the batch as a row-major pinhole image "
                     "(else it would sort the rays by entry point), records and replays the sample lists by itself",
            "hinted": "VolumeRenderer.forward(..., image_shape=(H, W))",
            "camera": "VolumeRenderer.render_persp (svox_t/renderer.py:310-366 -> volume_render_image, rt_kernel.cu:1153-1238): "
                      "the kernels generate the pinhole rays themselves, no ray tensors are read"}
    other = []
    if args.full and world == 1 and not args.no_plain:
        for oroute in ("hinted", "plain", "camera"):
            if oroute == args.route:
                continue
            for _ in range(3):
                step(route=oroute)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                step(route=oroute)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t1) / args.steps
            other.append({"route": oroute, "value": round(Q / dt / 1e6, 3), "unit": "Mrays/s",
                          "ms_per_step": round(dt * 1e3, 4), "what": WHAT[oroute]})

    def timed_with(attr, value, n_warm=3):
        old = getattr(_C, attr)
        setattr(_C, attr, value)
        try:
            for _ in range(n_warm):
                step()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t1) / args.steps
            routes = (_C.LAST_ROUTE["forward"], None if args.forward_only else _C.LAST_ROUTE["backward"])
        finally:
            setattr(_C, attr, old)
        return dt, routes

    # the opt-in tolerance modes, for the record (same process, after the timed region; `value` above is the exact mode)
    tolerance = None
    wide = fmt == "RGBA" and K in (8, 16, 32)
    if args.full and world == 1 and not args.no_plain and wide and not _C.NATIVE_MATH:
        # rows of 8 / 16 / 32 floats: bit-exact stepping, shading with v_exp_f32 / v_rcp_f32 (forward and backward)
        dt, routes = timed_with("NATIVE_MATH", True)
        tolerance = {"setting": "SVOXT_NATIVE_MATH=1", "value": round(Q / dt / 1e6, 3), "unit": "Mrays/s",
                     "ms_per_step": round(dt * 1e3, 4), "kernels": {"forward": routes[0], "backward": routes[1]},
                     "what": "the lists are the exact march's; exponentials and the quotients w / (1 + e) of the shade "
                             "kernels and of both sweeps of the per-tile backward with the hardware's v_exp_f32 / v_rcp_f32 "
                             "instead of the bit-exact expf replica and a double-precision divide: outputs within 1e-5 "
                             "relative (+1e-6), gradients within 1e-5 of the tight scale, tested at this size "
                             "(tests/test_gpu_query_and_misc.py::test_config4_native_math_tolerance_mode_full_size)"}
    elif args.full and world == 1 and not args.no_plain and not args.forward_only and _C.BWD_EXACT:
        # round 1's headline arithmetic: the backward that takes accum from the forward's output instead of
        # adding it up like the reference's first pass
        dt, _ = timed_with("BWD_EXACT", False)
        tolerance = {"setting": "SVOXT_BWD_EXACT=0", "value": round(Q / dt / 1e6, 3), "unit": "Mrays/s",
                     "ms_per_step": round(dt * 1e3, 4),
                     "what": "the single-march backward round 1's headline (BENCH_r01: 1038.5) was measured with: within "
                             "1e-5 of the summed magnitudes, but 36 % of the sigma-column entries differ from the "
                             "reference's by more than 1e-5 of their own value (tests/test_gpu_query_and_misc.py); "
                             "`value` above is the exact backward"}
    single_march = tolerance

    # BASELINE.json's other single-GPU configs, measured briefly in the SAME process (the headline workload with --full only),
    # so that whoever runs the full benchmark holds a number for them too and not just the builder's profiles
    # (VERDICT r04 "missing" 5).  Each: the hinted route, >= 0.25 s of untimed steps, then 20 steps between synchronizes.
    other_configs = None
    if args.full and world == 1 and args.workload == "d8_sh9_800" and not (args.no_plain or args.no_other_configs or args.forward_only or args.fast):
        def short(label, rend, feat, ry, shape, go, fwd_only, fast, q):
            def one():
                if fwd_only:
                    with torch.no_grad():
                        rend(feat, ry, image_shape=shape, fast=fast)
                else:
                    feat.grad = None
                    rend(feat, ry, image_shape=shape, fast=fast).backward(go)
            t0 = time.perf_counter()
            n0 = 0
            while time.perf_counter() - t0 < 0.25 or n0 < 10:
                one(); n0 += 1
                if n0 % 10 == 0:
                    torch.cuda.synchronize()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(20):
                one()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t1) / 20
            return {"config": label, "value": round(q / dt / 1e6, 3), "unit": "Mrays/s", "ms_per_step": round(dt * 1e3, 4),
                    "kernels": {"forward": _C.LAST_ROUTE["forward"], "backward": None if fwd_only else _C.LAST_ROUTE["backward"]}}
        other_configs = []
        try:
            other_configs.append(short("configs[2] with fast=True: 800x800, depth-8 SH9, forward+backward, thresholds 1e-2",
                                       renderer, features, rays, (H, W), gout, False, True, Q))
            tree.static_features = True
            other_configs.append(short("configs[1]: 800x800, depth-8 SH9, forward only (features declared static)",
                                       renderer, features, rays, (H, W), gout, True, False, Q))
            other_configs.append(short("configs[1] with fast=True (SURVEY 8(d)'s extra row)", renderer, features, rays, (H, W), gout, True, True, Q))
            tree.static_features = False
            d9, K9, fmt9, W9, H9 = WORKLOADS["d9_rgba32_1024"]
            st9 = synth.shell_tree(d9)
            tree9 = svox.N3Tree.from_arrays(st9.child, st9.data, st9.parent_depth, synth.shell_features(st9.n_features, K9),
                                            data_format=fmt9, device=dev)
            r9 = svox.VolumeRenderer(tree9)
            o9, d9_, v9 = synth.pinhole_rays(W9, H9, c2w=pose)
            rays9 = svox.Rays(o9.to(dev), d9_.to(dev), v9.to(dev))
            g9 = synth.grad_output(W9 * H9, K9).to(dev)
            other_configs.append(short("configs[3]: 1024x1024, depth-9 RGBA data_dim 32, forward+backward (exact)",
                                       r9, tree9.features, rays9, (H9, W9), g9, False, False, W9 * H9))
            tree9.static_features = True
            other_configs.append(short("configs[3], forward only (features declared static)", r9, tree9.features, rays9, (H9, W9), g9, True, False, W9 * H9))
            with torch.no_grad():
                t1 = time.perf_counter()
                for _ in range(20):
                    r9.render_depth(tree9.features, rays9, image_shape=(H9, W9))
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t1) / 20
            other_configs.append({"config": "configs[3]'s second output: render_depth [Q, 1]", "value": round(W9 * H9 / dt / 1e6, 3),
                                  "unit": "Mrays/s", "ms_per_step": round(dt * 1e3, 4)})
            del tree9, r9, rays9, g9
        except Exception as exc:                       # (never at the price of the headline's line)
            other_configs.append({"error": f"{exc.__class__.__name__}: {exc}"})

    if rank == 0:
        ms_per_step = elapsed * 1e3 / args.steps
        value = world * Q / (elapsed / args.steps) / 1e6
        res = {
            "metric": "Mrays/s fwd+bwd, 800×800 render, depth-8 SH9 N3Tree, 1→8 MI355X"
                      if args.workload == "d8_sh9_800" and not args.forward_only and not args.fast
                      else f"Mrays/s {'fwd' if args.forward_only else 'fwd+bwd'}, {args.workload}" + (", fast=True (thresholds 1e-2)" if args.fast else ""),
            "value": round(value, 3),
            "unit": "Mrays/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "prewarm": prewarm,
            "retimed": retimed,
            "ms_per_step": round(ms_per_step, 4),
            # the same K steps, per step, from the HIP events on the launch stream (forward: previous step's end -> this
            # step's forward end; backward: -> this step's backward end): one hiccup and K slow steps read differently here
            "value_median": round(world * Q / (_median(step_steps) * 1e-3) / 1e6, 3),
            "per_step_ms": {"forward": [round(x, 4) for x in fwd_steps], "backward": [round(x, 4) for x in bwd_steps],
                            "summary": {"forward": _spread(fwd_steps), "backward": _spread(bwd_steps), "step": _spread(step_steps)},
                            "note": "`value` = rays / mean WALL time per step of the barrier-bracketed region (what the driver's "
                                    "clock sees); `value_median` = rays / median of the per-step event times (forward + backward)"},
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": f"depth-{depth} shell N3Tree (n_internal {st.n_internal}, M {M}), "
                            f"{fmt} data_dim {K}, {W}x{H} pinhole rays per GPU, "
                            f"{'forward' if args.forward_only else 'forward+backward'}, "
                            f"step_size 1e-3, thresholds {'1e-2 (fast=True)' if args.fast else '0'}",
                "rays_per_gpu": Q,
                "route": args.route,
                "backward_arithmetic": None if args.forward_only else
                ("exact (every contribution the reference's formula)" if _C.BWD_EXACT else "single march (SVOXT_BWD_EXACT=0)"),
                "partitioning": "replicated tree, one camera (ray batch) per GPU"
                                + ("; all-gather of pixels under the backward; all-reduce of grad in row chunks on a "
                                   "side stream, waited for before the next step (every-step update); "
                                   "`accumulation_arrangement` has the overlapped form" if world > 1 else ""),
                "features": "declared static (inference: the sigma bitmask is built once)" if args.forward_only
                            else "updated every step (nothing derived from them is cached between steps)",
            },
            "kernel_ms": {"forward": round(fwd_ms, 4), "backward": round(bwd_ms, 4),
                          "forward_median": round(_median(fwd_steps), 4), "backward_median": round(_median(bwd_steps), 4)},
            "kernels": {"forward": route_fwd, "backward": route_bwd},
        }
        if args.full:
            ref_fwd, ref_bwd = reference_equivalent_bytes(cnt, Q, M, K, C)
            A = cnt[4]
            stride = K if (K <= 8 or K % 16 == 0) else (K + 15) // 16 * 16
            tree_bytes = 4 * touched.get("grid_cells", 0) + 8 * touched.get("node_pairs", 0) + \
                4 * (touched.get("child_words", 0) + touched.get("data_words", 0))
            recording = not args.forward_only
            fwd_parts = {
                "rays": 36 * Q, "pixels_written": 4 * (C + 1) * Q,
                "feature_rows_read": 4 * K * touched["rows_valid"], "tree_words_read": tree_bytes,
                "records_written": 8 * A if recording else 0, "aux_written": 16 * Q if recording else 0,
                # (att, e0, e1, e2) per sample, left by the recording forward for the exact backward
                "backward_terms_written": 16 * A if (recording and forward_terms) else 0,
            }
            if fmt == "RGBA" and K in (8, 16, 32) and _C.EXP_TABLE and not _C.NATIVE_MATH and "shade_chan" in (route_fwd or ""):
                # the exponentials table (svoxt_tree.exp_table): every forward that is not told the features are static
                # reads the feature table once and writes the table once; the shade then reads ITS rows (counted above)
                fwd_parts["exp_table_pass"] = 0 if args.forward_only else 2 * 4 * M * K
            bwd_parts = None
            kept_scratch = bool(_C.GRAD_SCRATCH and "render_bwd_kernel (marches" not in (route_bwd or ""))
            if not args.forward_only:
                bwd_parts = {
                    # (the padded scratch kept between steps is left zeroed by the row compaction: no fill of its own)
                    "grad_memset": 0 if (kept_scratch and stride != K) else 4 * M * stride,
                    "upstream_gradient_read": 4 * (C + 1) * Q, "aux_read": 16 * Q,
                    "rays": 36 * cnt[0], "records_read": 8 * A,
                    # with the forward's hand-over the backward reads 16 B per sample instead of the feature rows
                    "feature_rows_read": 0 if forward_terms else 4 * K * touched["rows_composited"],
                    "terms_read": 16 * A if forward_terms else 0,
                    "atomic_requests_64B": 64 * atomic_requests if atomic_requests else 4 * K * A,
                    # (read the padded rows, write the dense gradient, and -- kept scratch -- leave the padded rows zeroed again)
                    "row_compaction": (4 * M * stride + 4 * M * K + (4 * M * stride if kept_scratch else 0)) if stride != K else 0,
                }
                if "grad_wide_kernel" in (route_bwd or "") or "ONEPASS" in (route_bwd or ""):
                    # sweep 1 -> sweep 2: (attenuation,) second-pass total_color per sample, written and read
                    bwd_parts["sweep_handover"] = (16 if "grad_wide_kernel" in route_bwd else 8) * A
                if atomic_requests is None or not atomic_requests:
                    bwd_parts["atomic_requests_note"] = "one row per sample (this route has no counting instance)"
            # (the exponentials table of rows of 8 / 16 / 32 floats is an OVERHEAD pass -- the reference has none -- like the
            # sigma bitmask: carried per kernel below, no longer counted as compulsory: VERDICT r04 weak 3)
            exp_table_bytes = fwd_parts.pop("exp_table_pass", 0)
            fwd_bytes = sum(fwd_parts.values())
            bwd_bytes = sum(v for v in bwd_parts.values() if not isinstance(v, str)) if bwd_parts else 0
            # ---- per kernel: which kernel moves which of the items above
            fp, bp = fwd_parts, (bwd_parts or {})
            tiles = (Q + 63) // 64
            mask_bytes = 64 * M + M // 8 + (4 * (tiles * 24 + 512 + 17 * tiles + 514) if recording else 0)   # one line per row, the bits, the lists' tables
            assign, survey = {}, {}
            rf = route_fwd or ""
            if "fwd_roles_kernel" in rf:
                assign["mask"] = (0, mask_bytes, "forward")
                assign["roles"] = (fwd_bytes, 0, "forward")
                assign["finish"] = (0, 0, "forward")
                survey["roles"] = ref_fwd
            elif "march_rec_kernel" in rf:
                assign["exptab" if exp_table_bytes else "mask"] = (0, exp_table_bytes or mask_bytes, "forward")
                march_b = fp["rays"] + fp["tree_words_read"] + fp["records_written"] + fp["aux_written"] + M // 8
                assign["march"] = (march_b, 0, "forward")
                # the shade reads the lists back and the (table) rows, writes the pixels (and the backward's terms)
                assign["shade"] = (8 * A + 16 * Q + fp["feature_rows_read"] + fp["pixels_written"] + fp["backward_terms_written"], 0, "forward")
                survey["march"], survey["shade"] = None, ref_fwd           # (8(d) has no split: the whole forward against the shade, the larger one)
            else:
                assign["fwd"] = (fwd_bytes, 0, "forward")
                survey["fwd"] = ref_fwd
            if bwd_parts:
                rb = route_bwd or ""
                main = "fused" if "grad_fused" in rb else "wide" if "grad_wide" in rb else "bwd"
                zero_fill, compaction = bp.get("grad_memset", 0), bp.get("row_compaction", 0)
                assign[main] = (bwd_bytes - zero_fill - compaction, 0, "backward")
                survey[main] = ref_bwd - 4 * M * K
                if compaction:
                    # the dense [M, K] gradient is written once (the reference's zero-fill stands for it in 8(d)); reading the
                    # padded rows and clearing them again is this implementation's overhead
                    assign["compact"] = (4 * M * K, compaction - 4 * M * K, "backward")
                    survey["compact"] = 4 * M * K
                if zero_fill:
                    assign["fill"] = (zero_fill, 0, "backward")
                    survey["fill"] = 4 * M * K
            if args.forward_only or fwd_ms >= bwd_ms:
                dom, dom_kernel, dom_ms, dom_bytes, dom_ref = "forward", route_fwd, fwd_ms, fwd_bytes, ref_fwd
            else:
                dom, dom_kernel, dom_ms, dom_bytes, dom_ref = "backward", route_bwd, bwd_ms, bwd_bytes, ref_bwd
                dom_kernel += " + grad memset + row compaction"
            achieved = dom_bytes / (dom_ms * 1e-3) / 1e9
            prof_ok = world == 1 and not args.fast            # (committed profiles: N = 1, thresholds 0)
            traffic, traffic_note = pmc_traffic(args.workload, args.forward_only, dom) if prof_ok else \
                (None, "PMC profiles exist for N=1, thresholds 0 only")
            # Like with like: the chain floor of the STEPPING against the march kernel's own time (from the committed
            # kernel statistics of this command) when the forward is march + shade; the floor of stepping + shading
            # in one chain against the whole forward when it is one kernel.
            two_kernel = "march_rec" in (route_fwd or "")
            chain = "march" if two_kernel else "march+shade"
            kstats = kernel_stats_ms(args.workload, args.forward_only) if prof_ok else {}
            march_ms = next((v for k, v in kstats.items() if k.startswith("march_rec_kernel")), None)
            shade_ms = next((v for k, v in kstats.items() if k.startswith("shade_")), None)
            limits = {"forward": {
                "bound": "dependent chain of the longest ray (tree words -> step -> next tree words), not bytes",
                "longest_ray_crossings": touched["longest_ray_crossings"],
                "us_per_crossing_unloaded": US_PER_CROSSING_UNLOADED[chain],
                "floor_ms": round(touched["longest_ray_crossings"] * US_PER_CROSSING_UNLOADED[chain] * 1e-3, 4),
                "floor_of": "march_rec_kernel alone" if two_kernel else "render_fwd_kernel (stepping and shading in one chain)",
                "measured_ms": march_ms if two_kernel else round(fwd_ms, 4),
                "measured_of": (f"march_rec_kernel, profiles/{ROUND}_{args.workload}{'_fwd' if args.forward_only else ''}_kernel_stats.csv"
                                + ("" if march_ms is not None else " (not committed yet)")) if two_kernel
                               else "the whole forward (HIP events of this run)",
                "forward_ms_whole": round(fwd_ms, 4)}}
            if two_kernel and shade_ms is not None:
                limits["forward"]["shade_kernel_ms"] = shade_ms
            if atomic_requests:
                limits["backward"] = {
                    "bound": "floor: the rate at which the memory side takes 64-byte float-atomic requests (exp/atomic_bench.hip: 22 G/s)"
                             + (".  Not what binds the per-tile backward today: 15 % fewer requests (rows carried across the reduce's "
                                "16-record groups) made it 6 % SLOWER, shorter instruction paths in the same reduce 3 % faster -- its phases "
                                "are serial per workgroup and latency-bound (NOTEBOOK.md steps 39-41)"
                                if "grad_fused" in (route_bwd or "") else ""),
                    "atomic_requests": atomic_requests, "merged_rows": merged_rows,
                    "floor_ms": round(atomic_requests / ATOMIC_REQUESTS_PER_S * 1e3, 4), "measured_ms": round(bwd_ms, 4)}
            # What binds the dominant kernel group -- from this run's own numbers, not asserted: the working set of
            # configs 1-3 never leaves the Infinity Cache and the two big kernels sit at 0.13-0.29 of the HBM roofline, so
            # "hbm" would misname it.  forward: as long as the dependent chain of its longest ray
            # (+ the shading backlog) -> "latency"; per-tile backward of 3-channel payloads: a chain of barrier-separated
            # phases over an atomic-request floor it does not reach -> "latency"; backward of wide rows in exact mode:
            # vector ALU (the bit-exact expf replica and a double-precision divide per sigmoid) -> "valu".
            wide_exact = "grad_wide_kernel" in (route_bwd or "") and "native" not in (route_bwd or "")
            if dom == "backward" and wide_exact and "forward's table" not in (route_bwd or ""):
                bound, bound_detail = "valu", ("vector ALU: the exact sigmoids of both sweeps (pexpf + a double-precision divide each); "
                                               "rocprofv3 PMC of this command: SQ_INSTS_VALU per (sample, channel) in profiles/" + ROUND + "_*")
            elif dom == "backward" and wide_exact:
                lim = limits.get(dom, {})
                bound = "latency"
                bound_detail = ("barrier-separated phases per tile and window at four workgroups per CU: with the exponentials from the "
                                "forward's table the kernel waits 70 % of its wavefront-cycles (SQ_WAIT_ANY / SQ_WAVE_CYCLES, 11 % VALU "
                                "active: profiles/" + ROUND + "_d9_rgba32_1024_pmc_summary.txt); its atomic-request floor is %s ms of the %s measured"
                                % (lim.get("floor_ms"), lim.get("measured_ms")))
            else:
                lim = limits.get(dom, {})
                bound = "latency"
                bound_detail = (("the dependent chain of the longest ray: floor %(floor_ms)s ms against %(measured_ms)s measured" % lim)
                                if dom == "forward" else
                                ("barrier-separated phases per tile; its atomic-request floor is %s ms of the %s measured"
                                 % (lim.get("floor_ms"), lim.get("measured_ms"))))
            step_ref = ref_fwd + (0 if args.forward_only else ref_bwd)
            ktable = kernel_table(args.workload, args.forward_only, assign, survey, {"forward": fwd_ms, "backward": bwd_ms}, prof_ok)
            largest = next((r for r in ktable if r["ms"]), None)
            res.update({
                "counters": dict(zip(("rays_hit", "steps", "levels", "valid", "active"), cnt)),
                "touched": touched,
                "compulsory_bytes": {"forward": fwd_parts, "backward": bwd_parts,
                                     "overhead_passes": {k: v[1] for k, v in assign.items() if v[1]},
                                     "step_total": fwd_bytes + bwd_bytes,
                                     "step_gbps": round((fwd_bytes + bwd_bytes) / (ms_per_step * 1e-3) / 1e9, 2)},
                "roofline": {
                    "bound": bound,
                    "bound_detail": bound_detail,
                    "frac_of": "hbm (secondary: the fraction of the 8 TB/s HBM roofline the dominant group's compulsory bytes reach; "
                               "the group is bound by `bound`, see limits)",
                    "kernel": dom_kernel,
                    "achieved": round(achieved, 2),
                    "peak": HBM_PEAK_GBS,
                    "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 5),
                    "traffic": traffic,
                    "traffic_note": traffic_note,
                    # per kernel: the largest kernel first; `frac_largest_kernel` is ITS fraction of the HBM
                    # roofline (durations from this round's committed kernel statistics; null until those exist)
                    "kernels": ktable,
                    "frac_largest_kernel": None if largest is None else largest["frac"],
                    "largest_kernel": None if largest is None else largest["kernel"],
                    "frac_8d_note": "frac_8d > 1 in a row below: the kernel does not do the reference's work (sample lists replace two of "
                                    "its three marches, the grid its descent, the per-tile merge its per-sample atomics) -- the same route is "
                                    "held bit for bit (forward) / to 1e-5 of the tight scale (gradient) at full size by the tests",
                    "achieved_note": f"compulsory bytes of the {dom} as run (compulsory_bytes.{dom}: each item counted once, "
                                     "distinct rows / tree words / atomic requests counted on the device) / its mean duration "
                                     "from HIP events on the launch stream; the working set of this config sits in the 256 MiB "
                                     "Infinity Cache, so the fraction of the HBM roofline is low by construction: see limits",
                    "reference_equivalent_gbps": round(dom_ref / (dom_ms * 1e-3) / 1e9, 2),
                    "reference_equivalent_note": "SURVEY.md 8(d): the bytes the REFERENCE's algorithm moves for the same result "
                                                 "(a tree march per pass, 8 B per gradient float) / this kernel group's time",
                    # SURVEY.md 8(d)'s own figure for the WHOLE step, so that nobody has to recompute it: above 1 does not
                    # mean skipped work -- the sample lists replace two of the reference's three marches, the grid its
                    # descent, the per-tile merge its per-sample atomics; the same route is held bit for bit (forward) /
                    # to 1e-5 of the tight scale (gradient) at full size by tests/test_gpu_query_and_misc.py
                    "reference_equivalent": {"bytes_per_step": step_ref, "gbps": round(step_ref / (ms_per_step * 1e-3) / 1e9, 2),
                                             "frac_of_hbm_peak": round(step_ref / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                             "forward_bytes": ref_fwd, "backward_bytes": None if args.forward_only else ref_bwd},
                    # both kernel groups (the dominant one is whichever took longer in this run: at the headline config the
                    # two are within 2 % of each other and take turns)
                    "groups": {g: {"ms": round(ms_, 4), "compulsory_bytes": b_, "achieved": round(b_ / (ms_ * 1e-3) / 1e9, 2),
                                   "frac": round(b_ / (ms_ * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                                   "traffic": (pmc_traffic(args.workload, args.forward_only, g)[0] if prof_ok else None)}
                               for g, ms_, b_ in (("forward", fwd_ms, fwd_bytes), ("backward", bwd_ms, bwd_bytes)) if ms_ > 0.02 and b_ > 0},
                },
                "limits": limits,
            })
        if other:
            res["other_routes"] = other
            # the drop-in route's number at top level: `value` is the `config.route` route
            plain = next((o for o in other if o["route"] == "plain"), None)
            if plain is not None:
                res["value_plain"] = plain["value"]
                res["value_plain_note"] = ("the two calls the reference's own autograd function makes (svox_t/renderer.py:60-77), no "
                                           "argument the reference lacks; `value` is route '%s'" % args.route)
        if args.route == "plain":
            res["value_plain"] = round(value, 3)
        if other_configs is not None:
            res["other_configs"] = other_configs
        if single_march is not None:
            res["tolerance_mode"] = single_march
        if accumulation is not None:
            res["accumulation_arrangement"] = accumulation
        if exchange is not None:
            res["gradient_exchange"] = exchange
        if world > 1:
            res["multi_gpu_note"] = ("kernel_ms is the compute stream's forward / backward per step; ms_per_step - kernel "
                                     "time = exposed collectives + host; unmeasured on hardware by the builder (no 8-GPU node)")
        if args.full and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(st, feats, o, d, v, fmt, K, gout.cpu(), args.forward_only)
        print(json.dumps(res), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def cpu_baseline(st, feats, o, d, v, fmt, K, gout, forward_only):
    """The CPU oracle (oracle/, a restatement -- the reference's own CPU renderer
    asserts) on the same workload, all host cores (OpenMP)."""
    from oracle import oracle as O
    from svox_t_amd.helpers import DataFormat
    df = DataFormat(fmt)
    ot = O.Tree(feats.numpy(), st.data, st.child)
    opt = O.make_options(format=df.format, basis_dim=df.basis_dim)
    Q = o.shape[0]
    rays = (o.numpy(), d.numpy(), v.numpy())
    g = gout.numpy()
    reps, dt = 0, 0.0
    t0 = time.perf_counter()
    while dt < 10.0 and reps < 64:          # ~10 s of wall time on the host cores
        O.volume_render(ot, *rays, opt)
        if not forward_only:
            O.volume_render_backward(ot, *rays, opt, g)
        reps += 1
        dt = time.perf_counter() - t0
    return {
        "value": round(reps * Q / dt / 1e6, 4),
        "unit": "Mrays/s",
        "cores": O.num_threads(),
        "kind": "port",
        "sample": f"the full workload ({Q} rays, {'forward' if forward_only else 'forward+backward'}) "
                  f"x {reps} repetitions, {dt:.1f} s wall, OpenMP over rays on {O.num_threads()} threads",
    }


def dry_run(args, world, rank):
    """--dry-run: everything of the N-rank bench that is not a kernel, on CPU tensors over gloo -- rendezvous from the
    launcher's environment, one camera per rank, the pixel gather started after the forward, the gradient exchange
    (OverlappedGradReducer, both arrangements), the barrier-bracketed timed loop with the MAX over ranks, the one JSON
    line on rank 0.  The renderer is replaced by a differentiable stand-in of the same shapes (features [M, K], rays
    [Q, 3] -> [Q, C+1]); `value` therefore measures nothing and the line says so in `data`."""
    import datetime
    from svox_t_amd import parallel
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
    torch.manual_seed(0)
    M, K, C, Q = 3344, 4, 3, 64 * 64
    features = torch.randn(M, K, requires_grad=True)
    dirs = torch.nn.functional.normalize(torch.randn(Q, 3) + torch.tensor([0.0, 0.0, float(rank)]), dim=1)
    sel = torch.randint(0, M, (Q,))
    gout = torch.randn(Q, C + 1)

    def render():
        rows = features[sel]                                   # a gather of feature rows, a per-ray weight, a sigmoid
        w = 1.0 - torch.exp(-torch.relu(rows[:, K - 1:]) * dirs[:, 2:].abs())
        return torch.cat([w * torch.sigmoid(rows[:, :C]), w], dim=1)

    reducer = parallel.OverlappedGradReducer(dist, backend="gloo") if dist is not None else None
    gathered = torch.empty((world * Q, C + 1)) if dist is not None else None

    def step(accumulate=False):
        features.grad = None
        out = render()
        gather = parallel.gather_pixels_async(dist, gathered, out.detach(), backend="gloo") if dist is not None else None
        out.backward(gout)
        if dist is not None:
            reducer.start(features.grad)
            if not accumulate:
                reducer.wait()
            gather.wait()

    def timed(n, **kw):
        if reducer is not None:
            reducer.wait()
        if dist is not None:
            dist.barrier()
        t0 = time.perf_counter()
        for _ in range(n):
            step(**kw)
        if reducer is not None:
            reducer.wait()
        if dist is not None:
            dist.barrier()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el

    for _ in range(args.warmup):
        step()
    elapsed = timed(args.steps)
    acc = timed(args.steps, accumulate=True) if dist is not None else None
    ok = True
    if dist is not None:
        # the reduced gradient is the same on every rank, and the gathered pixels hold every rank's block
        g = features.grad.detach().clone()
        ref = g.clone()
        dist.broadcast(ref, src=0)
        ok = bool(torch.equal(g, ref)) and bool(torch.equal(gathered[rank * Q:(rank + 1) * Q], render().detach()))
        t = torch.tensor([1.0 if ok else 0.0])
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        ok = bool(t.item() == 1.0)
    if rank == 0:
        print(json.dumps({
            "metric": "dry run (no GPU, stand-in renderer): launch / rendezvous / collectives / timing only",
            "value": round(world * Q / (elapsed / args.steps) / 1e6, 3), "unit": "Mrays/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed * 1e3 / args.steps, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "dry-run: CPU tensors, gloo, stand-in renderer -- not a measurement",
            "config": {"workload": f"stand-in: features [{M}, {K}], {Q} rays per rank", "rays_per_gpu": Q},
            "collectives_consistent": ok,
            "accumulation_arrangement": None if acc is None else {"ms_per_step": round(acc * 1e3 / args.steps, 4)},
            "roofline": None, "cpu_baseline": None}), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
