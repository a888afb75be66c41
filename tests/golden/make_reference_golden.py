"""Regenerate tests/golden/reference_*.npz: what a host build of the REFERENCE's own ray kernels (oracle/ref.py, built
from the reference checkout named by SVOXT_REFERENCE) returns for three small scenes, one per kernel family -- SH with
three channels, RGBA, and a lobe format (SG).

    python tests/golden/make_reference_golden.py

Nothing of the reference's text is kept, only arrays: the inputs (tree tables, features, lobes, rays, options, upstream
gradient), the reference's outputs under both threshold sets (volume_render, opacity_render, render_depth) and its
float32 batch gradient (volume_render_backward: the sequential sum in ray order), and `portable_gap`: per output array
the worst |oracle with its portable expf - reference|, measured here on the CPU, oracle against reference -- never
against a kernel.  The reference's `expf` is the C library's in this build, so the oracle with use_libm_exp(True) must
return the recorded outputs bit for bit; the generator asserts it before it writes.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import oracle as O                                                  # noqa: E402
from oracle import ref as R                                                     # noqa: E402
from svox_t_amd import synth                                                    # noqa: E402
from tests.test_gpu_random_stress import random_rays, random_tree               # noqa: E402

RADIUS, CENTER = (0.7, 1.3, 0.9), (0.2, -0.1, 0.4)
STEP, BACKGROUND, THRESH = 2e-3, 0.5, 1e-2
Q = 300
SCENES = {                       # name: (data_format, K, seed)
    "sh4": ("SH4", 13, 21),
    "rgba": ("RGBA", 4, 22),
    "sg4": ("SG4", 13, 23),
}
OUTPUTS = ("render", "opacity", "depth")


def sg_lobes(n, seed):
    rng = np.random.default_rng(seed)
    ax = rng.standard_normal((n, 3))
    return np.concatenate([rng.uniform(0.5, 8.0, (n, 1)), ax / np.linalg.norm(ax, axis=1, keepdims=True)], 1).astype(np.float32)


def options(fmt, basis_dim, fast):
    th = THRESH if fast else 0.0
    return O.make_options(step_size=STEP, background_brightness=BACKGROUND, format=fmt, basis_dim=basis_dim, sigma_thresh=th, stop_thresh=th)


def run(module, tree, rays, opt):
    return dict(render=module.volume_render(tree, *rays, opt), opacity=module.opacity_render(tree, *rays, opt),
                depth=module.render_depth(tree, *rays, opt))


def main():
    import svox_t_amd as svox
    for name, (fmt, K, seed) in SCENES.items():
        # (random_tree builds the topology; the lobe scene's tree is built as SH4, which has the same 13 columns)
        t, feats = random_tree(seed, N=2, max_depth=4, data_format="SH4" if fmt == "SG4" else fmt, K=K, radius=RADIUS, center=CENTER)
        n = t.n_internal
        df = svox.DataFormat(fmt)
        extra = sg_lobes(df.basis_dim, seed) if fmt == "SG4" else None
        arrays = dict(child=t.child[:n].numpy().copy(), data=t.data[:n].numpy().copy(), parent_depth=t.parent_depth[:n].numpy().copy(),
                      features=feats.numpy(), offset=t.offset.numpy().copy(), scaling=t.invradius.numpy().copy(),
                      radius=np.float64(RADIUS), center=np.float64(CENTER), data_format=np.array(fmt),
                      format=np.int32(df.format), basis_dim=np.int32(df.basis_dim), step_size=np.float32(STEP),
                      background_brightness=np.float32(BACKGROUND), thresholds=np.float32([0.0, THRESH]))
        if extra is not None:
            arrays["extra"] = extra
        rays = tuple(np.ascontiguousarray(a.numpy()) for a in random_rays(300 + seed, Q, t))
        arrays.update(origins=rays[0], dirs=rays[1], vdirs=rays[2])
        tree = O.Tree(arrays["features"], arrays["data"], arrays["child"], offset=arrays["offset"], scaling=arrays["scaling"], extra=extra)
        for fast in (0, 1):
            opt = options(df.format, df.basis_dim, fast)
            ref = run(R, tree, rays, opt)
            O.use_libm_exp(True)
            try:
                libm = run(O, tree, rays, opt)
            finally:
                O.use_libm_exp(False)
            portable = run(O, tree, rays, opt)
            for k in OUTPUTS:
                assert np.array_equal(ref[k].view(np.uint32), libm[k].view(np.uint32)), (name, fast, k)
                arrays[f"{k}_{fast}"] = ref[k]
                arrays[f"portable_gap_{k}_{fast}"] = np.float64(np.abs(portable[k].astype(np.float64) - ref[k].astype(np.float64)).max())
        opt = options(df.format, df.basis_dim, 0)
        g = synth.grad_output(Q, arrays["render_0"].shape[1], seed=seed).numpy()
        arrays["grad_output"] = g
        arrays["grad"] = R.volume_render_backward(tree, *rays, opt, g)
        path = os.path.join(HERE, f"reference_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}: M {feats.shape[0]}, nodes {n}, {os.path.getsize(path)} bytes, "
              f"hits {np.count_nonzero(arrays['opacity_0'])}, non-zero gradient entries {np.count_nonzero(arrays['grad'])}, "
              f"portable_gap {({k + '_' + str(f): float(arrays[f'portable_gap_{k}_{f}']) for k in OUTPUTS for f in (0, 1)})}")


if __name__ == "__main__":
    main()
