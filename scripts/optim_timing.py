#!/usr/bin/env python3
"""The feature-table optimizers (csrc/svoxt_optim.hip: FeatureSGD / FeatureRMSprop / FeatureAdam, dense and lazy) against
torch.optim's fastest variant on the same GPU in the same process (fused=True where torch offers it, else foreach=True), on
the two benchmark tables

    D8: the headline table, 668 912 x 28 floats (synth depth 8, SH9)
    C4: the config-4 table, 4 738 568 x 32 floats (synth depth 9)

with gradients that have 10 %, 50 % and 100 % of their rows touched and, on D8, the gradient of one headline backward
(800 x 800 rays).  Per step: the median of `--reps` event timings of `--batch` steps each, after a warm-up; beside it the
bytes the traffic model says the step must move (4 (1 + f (2 + 2 s)) bytes an element, s state tables,
f the touched fraction, f = 1 dense) and the rate that makes; in brackets, for the lazy step, the time the host takes to
issue one step() and the time of the C entry alone called with arguments packed once (a small step can be bounded by the
host, not by the kernel: the bracket tells which).  Then the training loop of exp/train_loop_probe.py with
torch.optim.Adam(fused=True), FeatureAdam(lazy=False) and FeatureAdam() in turn.  Every step runs in a child process of
its own under a time limit; the first one that fails ends the run.

    python scripts/optim_timing.py [--reps 9] [--batch 10] [--only D8] [--limit 300]
"""
import argparse
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import svox_t_amd as svox                      # noqa: E402
from svox_t_amd import synth                   # noqa: E402

TABLES = {"D8": (668912, 28), "C4": (4738568, 32)}
KINDS = {"sgd": (svox.FeatureSGD, torch.optim.SGD, dict(lr=1e-3), 0),
         "sgd_momentum": (svox.FeatureSGD, torch.optim.SGD, dict(lr=1e-3, momentum=0.9), 1),
         "rmsprop": (svox.FeatureRMSprop, torch.optim.RMSprop, dict(lr=1e-3), 1),
         "adam": (svox.FeatureAdam, torch.optim.Adam, dict(lr=1e-3), 2)}
STEPS = ["table:" + k for k in KINDS] + ["loop"]


def timed(fn, reps, batch, host=False):
    """Median over reps of the device time of `batch` calls, per call, in ms; host: also the median time the host took
    to ISSUE a call (no synchronise inside the window): where the two agree the figure is the host's, not the kernel's."""
    for _ in range(batch):
        fn()
    torch.cuda.synchronize()
    ts, hs = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        for _ in range(batch):
            fn()
        hs.append((time.perf_counter() - t0) / batch * 1e3)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / batch)
    ts.sort()
    hs.sort()
    return (ts[len(ts) // 2], hs[len(hs) // 2]) if host else ts[len(ts) // 2]


def c_entry(opt, p, lazy):
    """The C entry alone with the arguments of the optimizer's next step packed once: no Python checks, no tensors made."""
    from svox_t_amd.csrc import _abi, _extras
    group = opt.param_groups[0]
    kind, keys = opt._kind(group), opt._tables(group)
    tabs = [opt.state[p][k].data_ptr() for k in keys] + [None, None]
    hyper = _abi._COptimHyper(**opt._hyper(group, 100))
    args = (_extras.OPTIM_KINDS[kind], p.data_ptr(), p.grad.data_ptr(), tabs[0], tabs[1], p.shape[0], p.shape[1], hyper, int(lazy),
            torch.cuda.current_stream().cuda_stream)
    fn = _abi._lib.svoxt_optim_step

    def call():
        if fn(*args) != 0:
            raise RuntimeError(_abi._lib.svoxt_last_error().decode())
    return call


def torch_fastest(cls, params, **kw):
    for variant in ("fused", "foreach"):
        try:
            return cls(params, **kw, **{variant: True}), variant
        except (RuntimeError, TypeError, ValueError):
            continue
    return cls(params, **kw), "default"


def headline_gradient(dev):
    """The gradient of one headline step (depth 8, SH9, 800 x 800 rays, an L2 loss), as exp/train_loop_probe.py takes it."""
    st = synth.shell_tree(8)
    feats = synth.shell_features(st.n_features, 28)
    tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, data_format="SH9", device=dev)
    o, d, v = (t.to(dev) for t in synth.pinhole_rays(800, 800, c2w=synth.camera_pose(azimuth_deg=20.0)))
    out = svox.VolumeRenderer(tree)(tree.features, svox.Rays(o, d, v))
    ((out[:, :3] - torch.rand((800 * 800, 3), device=dev)) ** 2).mean().backward()
    return tree.features.grad.detach().clone()


def run_table(name, kind, reps, batch):
    dev = torch.device("cuda:0")
    M, K = TABLES[name]
    ours_cls, torch_cls, kw, ns = KINDS[kind]
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = {}
    for f in (0.1, 0.5, 1.0):
        live = torch.rand((M, 1), device=dev, generator=gen) < f
        grads[f"{int(100 * f):3d} %"] = torch.randn((M, K), device=dev, generator=gen) * live
    if name == "D8":
        grads["real "] = headline_gradient(dev)
        assert tuple(grads["real "].shape) == (M, K)
    p_ours = [torch.nn.Parameter(torch.randn((M, K), device=dev, generator=gen)) for _ in range(2)]
    p_torch = torch.nn.Parameter(p_ours[0].detach().clone())
    dense, lazy = ours_cls([p_ours[0]], lazy=False, **kw), ours_cls([p_ours[1]], lazy=True, **kw)
    theirs, variant = torch_fastest(torch_cls, [p_torch], **kw)
    print(f"{name} [{M}, {K}] {kind}: torch.optim.{torch_cls.__name__}({variant}=True)", flush=True)
    for label, g in grads.items():
        f = float((g != 0).any(dim=1).float().mean())
        for p in p_ours + [p_torch]:
            p.grad = g
        t = {"dense": timed(dense.step, reps, batch), "torch": timed(theirs.step, reps, batch)}
        t["lazy"], host = timed(lazy.step, reps, batch, host=True)
        raw, raw_host = timed(c_entry(lazy, p_ours[1], True), reps, 10 * batch, host=True)
        model = {"dense": 4.0 * M * K * (3 + 2 * ns), "lazy": 4.0 * M * K * (1 + f * (2 + 2 * ns))}
        print(f"  rows touched {label} ({100 * f:5.1f} %):  dense {t['dense']:.4f} ms ({model['dense'] / 1e6:7.1f} MB, "
              f"{model['dense'] / t['dense'] / 1e6:6.0f} GB/s)  lazy {t['lazy']:.4f} ms ({model['lazy'] / 1e6:7.1f} MB, "
              f"{model['lazy'] / t['lazy'] / 1e6:6.0f} GB/s)  torch {t['torch']:.4f} ms ({model['dense'] / t['torch'] / 1e6:6.0f} GB/s)"
              f"  -> dense {t['torch'] / t['dense']:.2f}x  lazy {t['torch'] / t['lazy']:.2f}x torch's"
              f"   [lazy: the host issues a step() in {host:.4f} ms; svoxt_optim_step alone, 10x the calls per window: {raw:.4f} ms "
              f"(issued in {raw_host:.4f} ms)]", flush=True)


def run_loop(reps):
    """exp/train_loop_probe.py's loop: a new camera of four every step, an L2 loss, zero_grad, backward, step."""
    dev = torch.device("cuda:0")
    st = synth.shell_tree(8)
    feats = synth.shell_features(st.n_features, 28).to(dev)
    tree = svox.N3Tree.from_arrays(st.child, st.data, st.parent_depth, feats, data_format="SH9", device=dev)
    r = svox.VolumeRenderer(tree)
    cams = [svox.Rays(*[t.to(dev) for t in synth.pinhole_rays(800, 800, c2w=synth.camera_pose(azimuth_deg=a))])
            for a in (20.0, 50.0, 110.0, 200.0)]
    target = torch.rand((800 * 800, 3), device=dev)
    makers = {"no optimizer": lambda p: None,
              "torch.optim.Adam(fused=True)": lambda p: torch_fastest(torch.optim.Adam, [p], lr=1e-3)[0],
              "FeatureAdam(lazy=False)": lambda p: svox.FeatureAdam([p], lr=1e-3, lazy=False),
              "FeatureAdam()": lambda p: svox.FeatureAdam([p], lr=1e-3)}
    for label, make in makers.items():
        p = torch.nn.Parameter(feats.clone())
        opt = make(p)

        def step(i):
            out = r(p, cams[i % len(cams)])
            loss = ((out[:, :3] - target) ** 2).mean()
            p.grad = None
            loss.backward()
            if opt is not None:
                opt.step()

        for i in range(8):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(reps):
            step(i)
        torch.cuda.synchronize()
        print(f"loop D8 800 x 800, {label:30s}: {(time.perf_counter() - t0) / reps * 1e3:.3f} ms/step", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--limit", type=int, default=300, help="seconds a step's child process may take")
    ap.add_argument("--step", default="", help="(internal) run this one step in this process")
    a = ap.parse_args()
    if a.step:
        if a.step == "loop":
            return run_loop(max(40, 4 * a.reps))
        return run_table(a.only, a.step.split(":")[1], a.reps, a.batch)
    for name in TABLES:
        if a.only and a.only != name:
            continue
        for step in STEPS:
            if step == "loop" and name != "D8":
                continue
            rc = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--only", name,
                                 "--step", step, "--reps", str(a.reps), "--batch", str(a.batch)]).returncode
            if rc != 0:
                print(f"{name} {step}: ended with status {rc}; nothing further is run", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
