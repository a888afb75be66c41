"""`python3 bench.py --gpus N` as the driver types it (no launcher, no WORLD_SIZE): bench.py starts its own ranks as
child processes through torch.distributed.run and relays rank 0's ONE JSON line and the exit code (VERDICT r04
"missing" 1).  Rehearsed here on CPU with --dry-run (gloo, CPU tensors, a stand-in for the renderer): the launch, the
rendezvous on 127.0.0.1, the pixel gather, the gradient exchange in both arrangements, the barrier-bracketed timing
with the MAX over ranks and the line itself are the real code paths of parallel.py / bench.py; only the kernels are
not."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*argv, env=None):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                          timeout=600, cwd=ROOT, env=e)


@pytest.mark.parametrize("n", [1, 2])
def test_bench_self_launch_dry_run(n):
    p = _run("--gpus", str(n), "--steps", "3", "--warmup", "1", "--dry-run")
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout                      # ONE line on stdout, whatever the ranks and the launcher print
    r = json.loads(lines[0])
    assert r["n_gpus"] == n and r["steps"] == 3 and r["warmup"] == 1
    assert r["collectives_consistent"] is True
    assert r["unit"] == "Mrays/s" and r["scaling"] == "weak" and "dry-run" in r["data"]
    assert abs(r["value"] - n * 4096 / (r["ms_per_step"] * 1e-3) / 1e6) <= 2e-3 * r["value"] + 1e-3
    if n > 1:
        assert r["accumulation_arrangement"]["ms_per_step"] > 0


def test_bench_under_a_launcher_takes_the_launchers_world_size():
    """The driver's N > 1 form: torch.distributed.run starts bench.py with RANK / WORLD_SIZE set -- no second launch."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--steps", "2", "--warmup", "1", "--dry-run"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=e)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 2


def test_bench_without_a_gpu_fails_loudly():
    """No CPU fallback for the real bench: without a GPU (and without --dry-run) it exits non-zero and says why."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = _run("--steps", "1", "--warmup", "0")
    assert p.returncode != 0 and "GPU" in (p.stderr + p.stdout)


def test_dump_outputs_keeps_what_fits_and_a_seeded_row_sample_of_the_rest(tmp_path):
    """--dump-outputs' writer: float32 files within the budget; the smaller array whole, the larger one as rows drawn with a
    fixed seed, in order -- the same rows on every call, so that two builds can be compared file for file."""
    import numpy as np
    import torch

    import bench
    grad = torch.arange(50000, dtype=torch.float64)[:, None] * torch.ones(1, 28, dtype=torch.float64)   # row i holds i
    pix = torch.rand(4096, 4)
    budget = 1_000_000
    kept = bench.dump_outputs(str(tmp_path / "a"), {"grad_features": grad, "pixels": pix}, budget=budget)
    bench.dump_outputs(str(tmp_path / "b"), {"pixels": pix, "grad_features": grad}, budget=budget)
    files = sorted((tmp_path / "a").iterdir())
    assert [f.name for f in files] == ["grad_features.npy", "pixels.npy"]
    assert sum(f.stat().st_size for f in files) <= budget
    g, p = np.load(tmp_path / "a" / "grad_features.npy"), np.load(tmp_path / "a" / "pixels.npy")
    assert g.dtype == p.dtype == np.float32
    np.testing.assert_array_equal(p, pix.numpy())
    rows = g[:, 0].astype(np.int64)
    assert kept == {"pixels": 4096, "grad_features": len(rows)} and 0.9 * (budget - 4096 * 16) / 112 < len(rows) < 50000
    assert np.all(np.diff(rows) > 0) and np.all(g == rows[:, None])            # distinct rows of the input, in order
    for f in files:
        np.testing.assert_array_equal(np.load(f), np.load(tmp_path / "b" / f.name))
